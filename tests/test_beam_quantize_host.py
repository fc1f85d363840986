"""Beam-searched residual quantization on the host: the torch restatement (modules.beam_quantize) against the fp64
numpy reference, the collision-resolution rule (modules.tokenizer.collisions) against a plain-Python loop, the
tokenizer's and the model's new arguments, the declared C entry points and their host-side argument checks."""
import os
import re

import numpy as np
import pytest
import torch

import beam_quantize_support as S
from conftest import ROOT

INTEGER = (200, 16, 32, 3, 6, "integer", 107)
RANDOM = [c for c in S.GPU_CASES if c[5] == "random" and c[4] <= 16]


def _torch_run(c):
    from modules.beam_quantize import beam_quantize_torch
    x, cbs, ref = S.case(c)
    paths, err, res = beam_quantize_torch(torch.from_numpy(x), torch.from_numpy(cbs), c[4])
    assert paths.dtype == torch.int64 and err.dtype == torch.float32 and res.dtype == torch.float32
    assert paths.shape == (c[0], c[4], c[3]) and err.shape == (c[0], c[4]) and res.shape == (c[0], c[4], c[1])
    return x, cbs, ref, paths.numpy(), err.numpy(), res.numpy()


def test_restatement_is_the_reference_on_integers():
    assert INTEGER in S.GPU_CASES
    x, cbs, ref, paths, err, res = _torch_run(INTEGER)
    assert not ref["safe"].all(), "the integer case has ties"
    assert np.array_equal(paths, ref["paths"])
    assert np.array_equal(err.astype(np.float64), ref["err"]), "exact keys: bitwise"
    assert np.array_equal(res.astype(np.float64), ref["residual"])
    S.check_invariants(x, cbs, paths, err, res, ref["scale"])


@pytest.mark.parametrize("c", RANDOM, ids=S.case_id)
def test_restatement_matches_reference_on_safe_items(c):
    x, cbs, ref, paths, err, res = _torch_run(c)
    safe = ref["safe"]
    print(S.case_id(c), "safe share", safe.mean())
    assert safe.mean() >= S.MIN_SAFE_SHARE, safe.mean()
    assert np.array_equal(paths[safe], ref["paths"][safe])
    np.testing.assert_allclose(err[safe].astype(np.float64), ref["err"][safe], rtol=1e-4, atol=0)
    S.check_invariants(x, cbs, paths, err, res, ref["scale"])


def test_restatement_argument_errors():
    from modules.beam_quantize import beam_quantize_torch
    x, cb = torch.zeros(4, 16), torch.zeros(2, 8, 16)
    for width in (0, 9, 33):
        with pytest.raises(ValueError, match="width"):
            beam_quantize_torch(x, cb, width)
    with pytest.raises(ValueError, match="power of two"):
        beam_quantize_torch(torch.zeros(4, 48), torch.zeros(2, 8, 48), 2)
    with pytest.raises(ValueError, match="L <= 16"):
        beam_quantize_torch(x, torch.zeros(17, 8, 16), 2)


# ---------------------------------------------------------------------------------------------- collisions
@pytest.mark.parametrize("name", ["duplicates", "disjoint", "crowded"])
def test_resolve_equals_python_loop(name):
    from modules.tokenizer import collisions
    from modules.tokenizer.semids import dedup_rank
    paths = S.collision_fixtures()[name]
    want_ids, want_choice = S.resolve_ref(paths)
    ids, choice = collisions.resolve(torch.from_numpy(paths), int(paths.max()) + 1)
    assert ids.dtype == torch.int64 and choice.dtype == torch.int64
    assert np.array_equal(ids.numpy(), want_ids) and np.array_equal(choice.numpy(), want_choice)
    assert np.array_equal(ids.numpy(), paths[np.arange(paths.shape[0]), want_choice])
    before, after = S.n_collided(paths[:, 0]), S.n_collided(want_ids)
    assert int((dedup_rank(ids) > 0).sum()) == after <= before
    if name == "duplicates":
        assert before == 56 and after < before       # 8 vectors x 8 copies: every copy but the first collided
        assert sorted(want_choice[::8].tolist()) == list(range(8)), "the copies of a vector take its 8 paths in turn"
    elif name == "disjoint":
        assert before == 0 and not want_choice.any()
    else:
        assert 0 < after < before and want_choice.max() > 1
        # some round-r proposal was refused because the tuple was owned before the round began
        owned0 = {tuple(p) for p in paths[:, 0].tolist()}
        assert any(tuple(paths[i, 1]) in owned0 for i in range(paths.shape[0]) if want_choice[i] > 1)


def test_resolve_argument_errors():
    from modules.tokenizer import collisions
    with pytest.raises(ValueError, match="N, W, L"):
        collisions.resolve(torch.zeros(4, 3, dtype=torch.int64), 4)
    with pytest.raises(ValueError, match="64-bit"):
        collisions.resolve(torch.zeros(4, 2, 16, dtype=torch.int64), 4096)


class _Items:
    def __init__(self, x):
        self.x = x

    def __len__(self):
        return self.x.shape[0]

    def __getitem__(self, idx):
        return _Items(self.x[idx])


def _cpu_tokenizer():
    """A tokenizer whose encoder is the identity and whose greedy pass is the width-1 beam: CPU only."""
    from modules.tokenizer.semids import SemanticIdTokenizer
    tok = SemanticIdTokenizer(input_dim=16, output_dim=16, hidden_dims=[8], codebook_size=32, n_layers=3, n_cat_feats=0)
    _, cbs = S.make_inputs(1, 16, 32, 3, "random", 202)
    for l, layer in enumerate(tok.rq_vae.layers):
        layer.embedding.weight.data.copy_(torch.from_numpy(cbs[l]))
    tok.rq_vae.encode = lambda x: x

    class _Out:
        def __init__(self, ids):
            self.sem_ids = ids
    tok.rq_vae.get_semantic_ids = lambda x: _Out(tok.rq_vae.get_semantic_id_beams(x, 1).sem_ids[:, 0])
    return tok, cbs


def test_precompute_corpus_ids_defaults_and_beam():
    from modules.tokenizer.semids import dedup_rank
    tok, cbs = _cpu_tokenizer()
    x = S.duplicate_vectors(16, 201)
    items = _Items(torch.from_numpy(x))
    default = tok.precompute_corpus_ids(items).clone()
    assert default.shape == (64, 4)
    assert torch.equal(tok.precompute_corpus_ids(items, beam=1), default)
    assert torch.equal(tok.precompute_corpus_ids(items, shard=False, beam=1, resolve_collisions=False), default)
    ref = S.beam_ref(x, cbs, 8)
    best = tok.precompute_corpus_ids(items, beam=8)
    assert np.array_equal(best[:, :3].numpy(), ref["paths"][:, 0]), "an item's id is its best beam path"
    assert torch.equal(best[:, 3], dedup_rank(best[:, :3])) and int(best[:, 3].max()) == 7
    resolved = tok.precompute_corpus_ids(items, beam=8, resolve_collisions=True)
    assert np.array_equal(resolved[:, :3].numpy(), S.resolve_ref(ref["paths"])[0])
    assert int((resolved[:, 3] > 0).sum()) < int((best[:, 3] > 0).sum())
    assert tok.prefix_trie().depth == 4
    with pytest.raises(ValueError, match="beam >= 2"):
        tok.precompute_corpus_ids(items, resolve_collisions=True)
    with pytest.raises(ValueError, match="beam >= 1"):
        tok.precompute_corpus_ids(items, beam=0)


def _model(**kw):
    from modules.quantize import QuantizeForwardMode
    from modules.rqvae import RqVae
    cfg = dict(input_dim=24, embed_dim=8, hidden_dims=[16], codebook_size=4, codebook_kmeans_init=False,
               codebook_mode=QuantizeForwardMode.ROTATION_TRICK, n_layers=2, n_cat_features=0)
    cfg.update(kw)
    return RqVae(**cfg)


def test_get_semantic_id_beams_refuses_unsupported_models():
    from modules.quantize import QuantizeDistance
    x = torch.zeros(4, 24)
    with pytest.raises(ValueError, match="training mode"):
        _model().get_semantic_id_beams(x, 2)
    with pytest.raises(ValueError, match="k-means"):
        _model(codebook_kmeans_init=True).eval().get_semantic_id_beams(x, 2)
    m = _model().eval()
    m.layers[1].distance_mode = QuantizeDistance.COSINE
    with pytest.raises(ValueError, match="L2"):
        m.get_semantic_id_beams(x, 2)


def test_get_semantic_id_beams_cpu_path():
    from modules.rqvae import RqVaeBeamOutput
    m = _model().eval()
    m.encode = lambda x: x
    x, _ = S.make_inputs(20, 8, 4, 2, "random", 301)
    cbs = np.stack([l.embedding.weight.detach().numpy() for l in m.layers])
    out = m.get_semantic_id_beams(torch.from_numpy(x), 3)
    assert isinstance(out, RqVaeBeamOutput)
    assert out.sem_ids.shape == (20, 3, 2) and out.errors.shape == (20, 3) and out.residuals.shape == (20, 3, 8)
    ref = S.beam_ref(x, cbs, 3)
    assert np.array_equal(out.sem_ids.numpy()[ref["safe"]], ref["paths"][ref["safe"]]) and ref["safe"].any()
    assert list(m.state_dict().keys()) == list(_model().state_dict().keys())


def test_ops_refuse_cpu_tensors():
    from rqvae_hip import ops, RqHipError
    with pytest.raises(RqHipError, match="no CPU fallback"):
        ops.rq_quantize_beam(torch.zeros(4, 16), torch.zeros(2, 8, 16), 2)


# ---------------------------------------------------------------------------------------------- C ABI
def test_entry_points_declared_and_typed():
    from rqvae_hip import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rqvae_hip.h")).read(), flags=re.S)
    for name, nargs in (("rq_quantize_beam_workspace", 5), ("rq_quantize_beam", 14)):
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert name in _lib._SIGS and name in _lib.EXPORTED_SYMBOLS and len(_lib._SIGS[name][0]) == nargs
    import train_decoder
    assert train_decoder.TOKENIZER_BEAM == 1 and train_decoder.TOKENIZER_RESOLVE_COLLISIONS is False   # off by default


def test_argument_checks_run_on_the_host():
    """-22 before any device work: this runs on a machine without a GPU."""
    import ctypes
    from rqvae_hip import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("library not built (run __graft_entry__.build())")
    lib = _lib.load()
    assert lib.rq_abi_version() == 4
    p = ctypes.c_void_p(4096)   # never dereferenced: every call below fails its checks first

    def rc(B=4, D=16, K=8, L=2, W=2, x=p, cb=p, sq=p, paths=p, err=p):
        return lib.rq_quantize_beam(x, B, D, cb, sq, K, L, W, paths, err, None, None, 0, None)
    for kw, text in ((dict(W=0), b"W"), (dict(W=9), b"W"), (dict(K=64, W=33), b"W"), (dict(D=48), b"power of two"),
                     (dict(D=128), b"power of two"), (dict(D=4), b"power of two"), (dict(K=4097), b"K"),
                     (dict(L=17), b"L"), (dict(L=0), b"L"), (dict(B=-1), b"B"), (dict(x=None), b"null pointer"),
                     (dict(cb=None), b"null pointer"), (dict(sq=None), b"null pointer"),
                     (dict(paths=None), b"null pointer"), (dict(err=None), b"null pointer"),
                     (dict(x=ctypes.c_void_p(4100)), b"aligned")):
        assert rc(**kw) == -22, kw
        msg = lib.rq_last_error()
        assert b"rq_quantize_beam" in msg and text in msg, (kw, msg)
    assert rc(B=0) == 0, "an empty batch is a no-op"
    assert lib.rq_quantize_beam_workspace(65536, 64, 256, 3, 8) == 0   # all beam state stays on chip
