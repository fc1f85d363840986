"""rq_code_usage and rq_codebook_revive on the device: bitwise against numpy (np.add.at; the restatement of the
revival rule in codebook_support) and against the plain-torch CPU path of modules.codebook_revival.revive_; the
host-side argument checks; RqVae.track_usage / revive_dead_codes end to end."""
import numpy as np
import pytest
import torch

import codebook_support as S

pytestmark = pytest.mark.gpu


def _usage(ids, K, device, counts=None):
    from rqvae_hip import ops
    L = ids.shape[1]
    c = torch.zeros((L, K), dtype=torch.int64, device=device) if counts is None else counts
    ops.code_usage(torch.from_numpy(np.ascontiguousarray(ids)).to(device), c)
    return c


# (64, 2, 20000): 40,000 bins, past the 8,192-bin LDS histogram -> the per-wave aggregated global adds
@pytest.mark.parametrize("B,L,K", [(1, 1, 1), (257, 3, 32), (1000, 4, 300), (64, 2, 20000)])
def test_code_usage_matches_numpy(B, L, K, device):
    g = np.random.Generator(np.random.PCG64(B + K))
    ids = g.integers(0, K, size=(B, L)).astype(np.int64)
    assert np.array_equal(_usage(ids, K, device).cpu().numpy(), S.usage_ref(ids, K))


@pytest.mark.parametrize("B,L,K", [(5000, 3, 256), (5000, 2, 20000)])   # LDS and global path
def test_code_usage_one_hot_bin(B, L, K, device):
    """A collapsed codebook: every row on one code per level."""
    ids = np.tile(np.array([K - 1, 0, 7][:L], np.int64), (B, 1))
    got = _usage(ids, K, device).cpu().numpy()
    assert np.array_equal(got, S.usage_ref(ids, K)) and got.sum() == B * L and got.max() == B


@pytest.mark.parametrize("K", [16, 20000])
def test_code_usage_skips_out_of_range_ids(K, device):
    g = np.random.Generator(np.random.PCG64(K))
    ids = g.integers(-1, K + 1, size=(777, 2)).astype(np.int64)
    ids[:5, 0], ids[5:10, 1], ids[10, 0] = -1, K, np.iinfo(np.int64).min
    assert (ids == -1).any() and (ids == K).any()
    # counts sits inside a larger buffer: its neighbours on both sides stay untouched
    buf = torch.full((2 * K + 64,), 9, dtype=torch.int64, device=device)
    counts = buf[32:32 + 2 * K].view(2, K)
    counts.zero_()
    _usage(ids, K, device, counts)
    got = buf.cpu().numpy()
    assert np.array_equal(got[32:32 + 2 * K].reshape(2, K), S.usage_ref(ids, K))
    assert (got[:32] == 9).all() and (got[32 + 2 * K:] == 9).all()


def test_code_usage_accumulates_and_empty_batch(device):
    g = np.random.Generator(np.random.PCG64(1))
    a, b = (g.integers(0, 300, size=(n, 4)).astype(np.int64) for n in (1000, 333))
    c = _usage(a, 300, device)
    _usage(b, 300, device, c)
    _usage(np.zeros((0, 4), np.int64), 300, device, c)   # B == 0: a no-op
    assert np.array_equal(c.cpu().numpy(), S.usage_ref(b, 300, S.usage_ref(a, 300)))


def test_code_usage_graph_replay(device):
    """One captured call replayed 3 times adds exactly 3x (a single-node graph)."""
    from rqvae_hip import ops
    g = np.random.Generator(np.random.PCG64(2))
    ids_np = g.integers(0, 32, size=(257, 3)).astype(np.int64)
    ids = torch.from_numpy(ids_np).to(device)
    counts = torch.zeros((3, 32), dtype=torch.int64, device=device)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.code_usage(ids, counts)
    counts.zero_()
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(counts.cpu().numpy(), 3 * S.usage_ref(ids_np, 32))


# --------------------------------------------------------------------------------------------- revive
def _device_inputs(case, device):
    t = lambda a: torch.from_numpy(a.copy()).to(device)  # noqa: E731
    w = [t(case["weights"][l]) for l in range(case["L"])]
    m = v = None
    if case["exp_avg"] is not None:
        m = [t(case["exp_avg"][l]) for l in range(case["L"])]
        v = [t(case["exp_avg_sq"][l]) for l in range(case["L"])]
    return w, t(case["counts"]), t(case["res"]), m, v


def _stack(ts):
    return None if ts is None else np.stack([x.detach().cpu().numpy() for x in ts])


@pytest.mark.parametrize("name", [c[0] for c in S.REVIVE_CASES])
def test_codebook_revive_matches_restatement_and_cpu_path(name, device):
    from modules.codebook_revival import revive_
    from rqvae_hip import ops
    case = S.revive_case(name)
    w, counts, res, m, v = _device_inputs(case, device)
    revived, n = ops.codebook_revive(w, counts, res, case["min_count"], case["seed"], m, v)
    assert revived.dtype == torch.bool and n.dtype == torch.int64
    S.check_revived(case, _stack(w), _stack(m), _stack(v), revived.cpu().numpy(), n.cpu().numpy())
    assert np.array_equal(counts.cpu().numpy(), case["counts"])   # only read
    # the module entry point: device against the plain-torch CPU path, bit for bit
    gw, gc, gres, gm, gv = _device_inputs(case, device)
    cw, cc, cres, cm, cv = _device_inputs(case, torch.device("cpu"))
    gn = revive_(gw, gc, gres, min_count=case["min_count"], seed=case["seed"], exp_avg=gm, exp_avg_sq=gv)
    cn = revive_(cw, cc, cres, min_count=case["min_count"], seed=case["seed"], exp_avg=cm, exp_avg_sq=cv)
    assert torch.equal(gn.cpu(), cn) and not gc.any() and not cc.any()
    assert np.array_equal(S.bits(_stack(gw)), S.bits(_stack(cw)))
    if gm is not None:
        assert np.array_equal(S.bits(_stack(gm)), S.bits(_stack(cm)))
        assert np.array_equal(S.bits(_stack(gv)), S.bits(_stack(cv)))


def test_codebook_revive_argument_checks(device):
    """B < K, L = 17 and D = 6 are refused on the host, by the op and by the C entry point (-22 with a message,
    nothing launched: the pointers are never dereferenced)."""
    import ctypes
    from rqvae_hip import _lib, ops
    lib = _lib.load()

    def args(L, K, D, B):
        return ([torch.zeros(K, D, device=device) for _ in range(L)], torch.zeros(L, K, dtype=torch.int64, device=device),
                torch.zeros(L, B, D, device=device))
    for (L, K, D, B), msg_py, msg_c in (((1, 8, 4, 4), "B=4 < K=8", b"B >= K"), ((17, 2, 4, 2), "L <= 16", b"L <= 16"),
                                        ((1, 2, 6, 2), "D % 4", b"D % 4")):
        w, counts, res = args(L, K, D, B)
        before = [x.clone() for x in w]
        with pytest.raises(ValueError, match=msg_py):
            ops.codebook_revive(w, counts, res, 1, 0)
        tab = (ctypes.c_void_p * L)(*[x.data_ptr() for x in w])
        revived = torch.full((L, K), 7, dtype=torch.uint8, device=device)
        n = torch.full((L,), 7, dtype=torch.int64, device=device)
        ws = torch.zeros(1024, dtype=torch.uint8, device=device)
        rc = lib.rq_codebook_revive(tab, None, None, L, K, D, _lib.ptr(counts), 1, _lib.ptr(res), B, 0, _lib.ptr(revived),
                                    _lib.ptr(n), _lib.ptr(ws), 1024, None)
        assert rc == -22 and msg_c in lib.rq_last_error(), lib.rq_last_error()
        torch.cuda.synchronize()
        assert (revived == 7).all() and (n == 7).all() and all(torch.equal(a, b) for a, b in zip(w, before))
    assert lib.rq_codebook_revive_workspace(17, 2) == 0 and lib.rq_codebook_revive_workspace(2, 300) >= 2 * 2 * 4
    rc = lib.rq_code_usage(None, 4, 0, 8, None, None)
    assert rc == -22 and b"rq_code_usage" in lib.rq_last_error()


# ---------------------------------------------------------------------------------- model, end to end
def _small_model(device):
    """The RqVae of __graft_entry__.smoke (ROTATION_TRICK, no k-means init, K = 32, D = 16, L = 3) with level
    codebooks of scale 2 and inputs of norm 32, so that encoder outputs and codewords are O(1) apart."""
    import gen_inputs as gi
    from modules.quantize import QuantizeForwardMode
    from modules.rqvae import RqVae
    inp, hid, D, K, L, B = 96, [64, 32], 16, 32, 3, 128
    st = {f"encoder.mlp.{2 * j}.weight": w for j, w in enumerate(gi.mlp_weights([inp] + hid + [D], 1))}
    st.update({f"decoder.mlp.{2 * j}.weight": w for j, w in enumerate(gi.mlp_weights([D] + hid[::-1] + [inp], 2))})
    st.update({f"layers.{l}.embedding.weight": gi.residual_rows(K, D, 10 + l, 2.0) for l in range(L)})
    model = RqVae(inp, D, hid, K, codebook_kmeans_init=False, codebook_mode=QuantizeForwardMode.ROTATION_TRICK,
                  n_layers=L, n_cat_features=0).to(device)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in st.items()})
    x = (gi.items(B, inp, 7) * np.float32(32)).astype(np.float32)
    return model, st, x


def test_revived_codes_are_selected_by_their_donors(device):
    """Track one training forward, revive, and tokenize again: at level 0 every revived code k is the id of its
    donor row (the codeword IS that row's encoder output, so its distance is 0 up to the rounding of the
    |x|^2 + |c|^2 - 2 x.c expansion). Input seed 7 / revival seed 2024, checked on the CPU with oracle/quantize.py
    (the block below repeats the check): 19 of the 32 level-0 codes are dead; every row's best level-0 code beats
    the runner-up by >= 7.2e-3 in squared distance (so the dead set cannot flip by rounding); after the revival
    the nearest OTHER level-0 codeword of every donor is >= 0.29 away (> 1e-3). The AdamW moment rows of revived
    codes are zero afterwards, every other moment row keeps its bits."""
    from data.schemas import SeqBatch
    from oracle import quantize as Q
    from oracle import rqvae as R
    from rqvae_hip import optim as hip_optim
    seed = 2024
    model, st, x = _small_model(device)
    K, B = 32, x.shape[0]
    # the recorded CPU check
    z, _ = R.mlp_fwd(x, [st[f"encoder.mlp.{2 * j}.weight"] for j in range(3)], normalize=False)
    d = np.sort(Q.l2_dist(z, st["layers.0.embedding.weight"]), 1)
    ids_cpu = Q.argmin_first(Q.l2_dist(z, st["layers.0.embedding.weight"]))
    dead_cpu = np.flatnonzero(np.bincount(ids_cpu, minlength=K) == 0)
    rows_cpu = S.donor_rows(seed, 0, dead_cpu.size, B)
    cb = st["layers.0.embedding.weight"].copy()
    cb[dead_cpu] = z[rows_cpu]
    d2 = Q.l2_dist(z[rows_cpu], cb)
    d2[np.arange(dead_cpu.size), dead_cpu] = np.inf
    assert len({r.tobytes() for r in x}) == B and dead_cpu.size >= 1
    assert (d[:, 1] - d[:, 0]).min() > 1e-3 and d2.min() > 1e-3

    opt = hip_optim.AdamW(model.parameters(), lr=0.0, weight_decay=0.0)   # lr 0: moments form, parameters stay
    xt = torch.from_numpy(x).to(device)
    model.train()
    model.track_usage()
    model(SeqBatch(None, None, None, xt, None, None), gumbel_t=0.2).loss.backward()
    opt.step()
    counts = model.code_usage.cpu().numpy().copy()
    assert counts.sum(1).tolist() == [B] * 3
    dead0 = np.flatnonzero(counts[0] == 0)
    assert np.array_equal(dead0, dead_cpu)
    weights = [layer.embedding.weight for layer in model.layers]
    before = [(w.detach().cpu().numpy().copy(), opt.state[w]["exp_avg"].cpu().numpy().copy(),
               opt.state[w]["exp_avg_sq"].cpu().numpy().copy()) for w in weights]
    assert all(np.abs(b[1]).sum() > 0 for b in before)

    n = model.revive_dead_codes(xt, seed=seed, optimizer=opt)
    assert model.training and not model.code_usage.any()
    assert n.tolist() == [int((counts[l] == 0).sum()) for l in range(3)]
    for l, w in enumerate(weights):
        dead = counts[l] == 0
        for got, old in zip((w.detach(), opt.state[w]["exp_avg"], opt.state[w]["exp_avg_sq"]), before[l]):
            assert np.array_equal(S.bits(got.cpu().numpy()[~dead]), S.bits(old[~dead]))
        assert not S.bits(opt.state[w]["exp_avg"].cpu().numpy()[dead]).any()
        assert not S.bits(opt.state[w]["exp_avg_sq"].cpu().numpy()[dead]).any()
    model.eval()
    with torch.no_grad():
        ids = model.get_semantic_ids(xt).sem_ids.cpu().numpy()
    assert np.array_equal(ids[S.donor_rows(seed, 0, dead0.size, B), 0], dead0)
    used, ppl = model.usage_stats()
    assert used == [0.0] * 3 and ppl == [0.0] * 3   # eval forwards do not count
