"""rq_quantize_beam on the device against the fp64 numpy reference (beam_quantize_support): bitwise on the integer
cases (exact keys, frequent ties), on every safe item of the random cases, the invariants of every case (W = 32
included), W = 1 against the greedy kernel, run-to-run and graph-replay determinism, the model's and the tokenizer's
use of it."""
import numpy as np
import pytest
import torch

import beam_quantize_support as S
import beam_support as bs
import gen_inputs as gi

pytestmark = pytest.mark.gpu

_RUNS = {}


def _bits(t):
    return t.contiguous().view(torch.int32)


def _run(c, device):
    """The op's outputs of one case (device tensors), computed once and shared."""
    from rqvae_hip import ops
    if c not in _RUNS:
        x, cbs, _ = S.case(c)
        _RUNS[c] = ops.rq_quantize_beam(torch.from_numpy(x).to(device), torch.from_numpy(cbs).to(device), c[4],
                                        with_residuals=True)
    return _RUNS[c]


@pytest.mark.parametrize("c", S.GPU_CASES, ids=S.case_id)
def test_against_reference(device, c):
    B, D, K, L, W, kind, _ = c
    x, cbs, ref = S.case(c)
    paths_t, err_t, res_t = _run(c, device)
    assert paths_t.shape == (B, W, L) and paths_t.dtype == torch.int64
    assert err_t.shape == (B, W) and err_t.dtype == torch.float32 and res_t.shape == (B, W, D)
    paths, err, res = paths_t.cpu().numpy(), err_t.cpu().numpy(), res_t.cpu().numpy()
    safe = ref["safe"]
    print(S.case_id(c), "safe share", safe.mean(), "paths equal on", (paths == ref["paths"]).all((1, 2)).mean())
    if kind == "integer":
        assert np.array_equal(paths, ref["paths"])
        assert np.array_equal(err.astype(np.float64), ref["err"]), "exact keys: bitwise"
        assert np.array_equal(res.astype(np.float64), ref["residual"])
    elif W <= 16:
        assert safe.mean() >= S.MIN_SAFE_SHARE, safe.mean()
        assert np.array_equal(paths[safe], ref["paths"][safe])
        np.testing.assert_allclose(err[safe].astype(np.float64), ref["err"][safe], rtol=1e-4, atol=0)
    S.check_invariants(x, cbs, paths, err, res, ref["scale"])


@pytest.mark.parametrize("c", [S.GPU_CASES[1], S.GPU_CASES[5], S.GPU_CASES[7]], ids=S.case_id)
def test_two_calls_give_identical_bits(device, c):
    from rqvae_hip import ops
    x, cbs, _ = S.case(c)
    first = _run(c, device)
    again = ops.rq_quantize_beam(torch.from_numpy(x).to(device), torch.from_numpy(cbs).to(device), c[4], True)
    assert torch.equal(first[0], again[0])
    assert torch.equal(_bits(first[1]), _bits(again[1])) and torch.equal(_bits(first[2]), _bits(again[2]))
    no_res = ops.rq_quantize_beam(torch.from_numpy(x).to(device), torch.from_numpy(cbs).to(device), c[4])
    assert len(no_res) == 2 and torch.equal(no_res[0], first[0]) and torch.equal(_bits(no_res[1]), _bits(first[1]))


@pytest.mark.parametrize("c", S.GPU_CASES, ids=S.case_id)
def test_width_one_is_the_greedy_rule(device, c):
    from rqvae_hip import ops
    B, D, K, L, _, kind, _ = c
    x, cbs, _ = S.case(c)
    ref = S.beam_ref(x, cbs, 1)          # its safe flag is the top-2 gap of every level
    xd, cd = torch.from_numpy(x).to(device), torch.from_numpy(cbs).to(device)
    paths, err = ops.rq_quantize_beam(xd, cd, 1)
    greedy = ops.rq_quantize(xd, cd, ops.MODE_EVAL)[2]
    keep = np.ones(B, bool) if kind == "integer" else ref["safe"]
    assert keep.mean() >= S.MIN_SAFE_SHARE
    assert np.array_equal(paths.cpu().numpy()[keep, 0], greedy.cpu().numpy()[keep])
    assert np.array_equal(paths.cpu().numpy()[keep, 0], ref["paths"][keep, 0])
    np.testing.assert_allclose(err.cpu().numpy()[keep, 0].astype(np.float64), ref["err"][keep, 0], rtol=1e-4,
                               atol=1e-5 * float(ref["scale"].max()))


def test_graph_replay_gives_the_same_bits(device):
    from rqvae_hip import ops
    c = S.GPU_CASES[1]
    x, cbs, _ = S.case(c)
    want = _run(c, device)
    xd, cd = torch.from_numpy(x).to(device), torch.from_numpy(cbs).to(device)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = ops.rq_quantize_beam(xd, cd, c[4], with_residuals=True)
    for t in got:
        t.zero_()
    for _ in range(2):
        graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(got[0], want[0])
    assert torch.equal(_bits(got[1]), _bits(want[1])) and torch.equal(_bits(got[2]), _bits(want[2]))


def test_argument_errors(device):
    from rqvae_hip import ops
    x, cb = torch.zeros(4, 16, device=device), torch.zeros(2, 8, 16, device=device)
    for width in (0, 9):
        with pytest.raises(ValueError, match="width"):
            ops.rq_quantize_beam(x, cb, width)
    with pytest.raises(ValueError, match="power of two"):
        ops.rq_quantize_beam(torch.zeros(4, 128, device=device), torch.zeros(2, 8, 128, device=device), 2)
    paths, err = ops.rq_quantize_beam(x[:0], cb, 2)
    assert paths.shape == (0, 2, 2) and err.shape == (0, 2)


# ---------------------------------------------------------------------------------------------- model / tokenizer
INP, HID, D, K, L = 96, [64, 32], 16, 32, 3


def _state(seed):
    st = {f"encoder.mlp.{2 * j}.weight": w for j, w in enumerate(gi.mlp_weights([INP] + HID + [D], seed))}
    st.update({f"decoder.mlp.{2 * j}.weight": w for j, w in enumerate(gi.mlp_weights([D] + HID[::-1] + [INP], seed + 1))})
    st.update({f"layers.{l}.embedding.weight": gi.residual_rows(K, D, seed + 10 + l, 0.5 * 0.6 ** l) for l in range(L)})
    return {k: torch.from_numpy(v) for k, v in st.items()}


def test_model_beams_equal_the_op(device):
    from modules.rqvae import RqVae, RqVaeBeamOutput
    from rqvae_hip import ops
    model = RqVae(INP, D, HID, K, codebook_kmeans_init=False, n_layers=L, n_cat_features=0).to(device).eval()
    model.load_state_dict(_state(7))
    x = torch.from_numpy(gi.items(150, INP, 3)).to(device)
    out = model.get_semantic_id_beams(x, 5)
    assert isinstance(out, RqVaeBeamOutput) and out.sem_ids.shape == (150, 5, L)
    with torch.no_grad():
        cbs = torch.stack([layer.embedding.weight for layer in model.layers])
        paths, err, res = ops.rq_quantize_beam(model.encode(x), cbs, 5, with_residuals=True)
    assert torch.equal(out.sem_ids, paths)
    assert torch.equal(_bits(out.errors), _bits(err)) and torch.equal(_bits(out.residuals), _bits(res))
    greedy = model.get_semantic_ids(x).sem_ids
    same = (greedy == out.sem_ids[:, 0]).all(1).float().mean().item()
    print("best beam path == greedy path on", same)
    model.train()
    with pytest.raises(ValueError, match="training mode"):
        model.get_semantic_id_beams(x, 5)


def test_tokenizer_resolves_duplicates_and_decodes(golden, device):
    from modules.tokenizer.semids import SemanticIdTokenizer, dedup_rank
    tok = SemanticIdTokenizer(input_dim=INP, output_dim=D, hidden_dims=HID, codebook_size=K, n_layers=L, n_cat_feats=0)
    tok.rq_vae.load_state_dict(_state(7))
    tok = tok.to(device)
    x = np.tile(gi.items(8, INP, 5), (8, 1))                     # 8 vectors x 8 copies
    items = bs.Items(x)
    plain = tok.precompute_corpus_ids(items).clone()
    best = tok.precompute_corpus_ids(items, beam=8).clone()
    ids = tok.precompute_corpus_ids(items, beam=8, resolve_collisions=True)
    tok.rq_vae.eval()   # precompute_corpus_ids restores the tokenizer's own (training) mode on its way out
    paths = tok.rq_vae.get_semantic_id_beams(torch.from_numpy(x).to(device), 8).sem_ids.cpu().numpy()
    want, choice = S.resolve_ref(paths)
    want = torch.from_numpy(want)
    assert torch.equal(ids.cpu(), torch.cat([want, dedup_rank(want).unsqueeze(1)], 1))
    assert np.array_equal(best[:, :L].cpu().numpy(), paths[:, 0])
    n_plain, n_best, n_res = (int((t[:, L] > 0).sum()) for t in (plain, best, ids))
    print("items with dedup rank > 0: greedy", n_plain, "beam", n_best, "resolved", n_res)
    assert n_plain >= 56 and n_best >= 56 and n_res < n_best and n_res == S.n_collided(want.numpy())
    # the trie and the search downstream are unchanged
    trie = tok.prefix_trie()
    assert trie.depth == L + 1 and trie.leaf_item.numel() == 64   # with the dedup column every row is distinct
    z = golden("generation")
    model = bs.decoder_model(z, device, dropout=0.0, scale_out=float(z["out_proj_scale"]))
    model.enable_generation = True
    model.inference_prefix_index = tok
    rec = model.recommend(bs.tokenized(z, device), k=10)
    got, rows = rec.item_ids.cpu(), rec.sem_ids.cpu()
    live = got >= 0
    assert live.any() and (got[live] < 64).all()
    assert torch.equal(ids.cpu()[got[live]], rows[live]), "cached_ids[item_ids] == sem_ids: only corpus ids"
