"""Semantic-ID tokenizer — drop-in for reference modules/tokenizer/semids.py (SemanticIdTokenizer
:23-154; same constructor, `cached_ids` layout (N, L+1) with the dedup column, forward contract).

MI355X path:
  * corpus ids: the frozen RqVae's eval-mode fused quantize kernel over the whole corpus in large
    device batches (the reference walks 512-item batches); with `shard=True` under data
    parallelism each rank quantizes its contiguous slice and the ids are all-gathered,
    the dedup column is then computed on the gathered corpus (identical on every rank);
  * dedup column (`semids.py:84-99`: for each item, the number of EARLIER items with the same
    L-tuple): one stable device sort of packed tuple keys + a segmented rank, O(N log N) instead
    of the reference's O(N^2) all-pairs comparison — identical values;
  * `precompute_corpus_ids(beam=, resolve_collisions=)` (this build's addition, off by default): ids from the beam
    encoder (an item's best of `beam` code paths) and, asked to, a colliding item moved to its next-best path
    (modules/tokenizer/collisions.py) before the dedup column is computed;
  * `exists_prefix`: sorted packed-prefix keys + binary search (torch.searchsorted) instead of
    the O(P x N) broadcast compare. `reference_batching=True` (default) reproduces the reference's
    batching quirk (`math.ceil(n // 16)` skips the last partial batch of 16 prefixes, which then
    report False; SURVEY A-12) so generation matches the reference; pass False for the fixed
    behaviour;
  * `prefix_trie` / `trie_index` / `blocked_nodes` (this build's additions): the corpus ids as a level-by-level CSR
    trie for constrained decoding, and per batch of item-id histories the trie nodes whose leaves are all listed
    (seen-item exclusion) — one HIP launch on the device, plain torch on the CPU;
  * `item_filter` (this build's addition): per group of a bool item mask the ItemFilter tables — every level's bitmap
    of nodes that still lead to an allowed item, and every leaf's lowest allowed item (catalogue filters: "only what
    is in stock") — two HIP launches on the device, plain torch on the CPU;
  * `item_bias` (this build's addition): per group of an fp32 per-item score adjustment the ItemBias tables — every
    level's per-node bound (the largest adjustment of an item below the node) and every leaf's item that attains it
    (promotions, de-biasing, priors: "rank by the model's score plus an adjustment") — two HIP launches on the device,
    plain torch on the CPU.
"""
import math
from typing import List, NamedTuple, Optional

import torch
from torch import nn
from torch import Tensor

from data.schemas import SeqBatch, TokenizedSeqBatch
from modules.rqvae import RqVae
from modules.utils import eval_mode
from rqvae_hip import dp

BATCH_SIZE = 16
CORPUS_BATCH = 65536


def _pack(cols: Tensor, base: int) -> Tensor:
    """Rows of small non-negative ints -> int64 keys (lexicographic order preserved)."""
    key = torch.zeros(cols.shape[:-1], dtype=torch.int64, device=cols.device)
    for j in range(cols.shape[-1]):
        key = key * base + cols[..., j].to(torch.int64)
    return key


def dedup_rank(ids: Tensor) -> Tensor:
    """rank[i] = #{j < i : ids[j] == ids[i]} for an (N, L) integer tensor (stable sort + segmented rank)."""
    n = ids.shape[0]
    if n == 0:
        return torch.zeros(0, dtype=torch.int64, device=ids.device)
    base = int(ids.max().item()) + 1
    key = _pack(ids, base)
    sk, order = torch.sort(key, stable=True)
    pos = torch.arange(n, device=ids.device)
    first = torch.ones(n, dtype=torch.bool, device=ids.device)
    first[1:] = sk[1:] != sk[:-1]
    start = torch.cummax(torch.where(first, pos, torch.zeros_like(pos)), dim=0).values
    rank = torch.empty(n, dtype=torch.int64, device=ids.device)
    rank[order] = pos - start
    return rank


class PrefixTrie(NamedTuple):
    """Level-by-level CSR trie of the corpus ids (SemanticIdTokenizer.prefix_trie). Level p holds the sorted unique
    length-p prefixes (prefix_table(p)'s keys, in that order); level 0 is the single root."""
    tok: tuple          # tok[p], p = 1..depth: int32 (n_p), the last token of each level-p node (tok[0] is None)
    child_off: tuple    # child_off[p], p = 0..depth-1: int32 (n_p + 1), node i's children in level p + 1 are
                        # [child_off[p][i], child_off[p][i + 1]): contiguous, ascending by token
    leaf_item: Tensor   # int64 (n_depth): the lowest corpus index whose row is that level-depth path
    depth: int
    base: int


class TrieIndex(NamedTuple):
    """Per-item and per-leaf views of the PrefixTrie (SemanticIdTokenizer.trie_index), for seen-item exclusion."""
    item_leaf: Tensor   # int32 (N): each corpus item's leaf (level-depth node); items with equal rows share it
    leaf_anc: tuple     # leaf_anc[q - 1], q = 1..depth: int32 (n_depth), each leaf's level-q ancestor (non-decreasing;
                        # the last one is the leaf itself)
    leaf_count: tuple   # leaf_count[q - 1], q = 1..depth: int32 (n_q), each level-q node's number of leaves


class ItemFilter(NamedTuple):
    """A catalogue filter over the PrefixTrie (SemanticIdTokenizer.item_filter): per group of an item mask, which
    nodes of every level still lead to an allowed item. Built once, reused across calls."""
    bits: tuple         # bits[q - 1], q = 1..depth: int32 (G, ceil(n_q / 32)); bit c & 31 of word c >> 5 in row g is
                        # set iff the level-q node c has at least one allowed item below it in group g
    leaf_item: Tensor   # int64 (G, n_depth): the lowest ALLOWED corpus index whose row is that leaf, -1 if none
    groups: int         # G


class ItemBias(NamedTuple):
    """A per-item score bias over the PrefixTrie (SemanticIdTokenizer.item_bias): per group of a bias table, the most
    any item below each node of every level adds to its score. Built once, reused across calls."""
    upper: tuple        # upper[q - 1], q = 1..depth: fp32 (G, n_q); row g holds every level-q node's bound, the largest
                        # (cleaned) bias[g][i] of an item i below it, -inf if it has none
    leaf_item: Tensor   # int64 (G, n_depth): the lowest corpus index among the items on that leaf that attain its
                        # bound, -1 where the bound is -inf
    groups: int         # G


_NO_NODE = torch.iinfo(torch.int32).max   # padding of blocked_nodes' rows


class SemanticIdTokenizer(nn.Module):
    """Tokenizes sequences of item features into sequences of semantic ids (L codewords + dedup)."""

    def __init__(self, input_dim: int, output_dim: int, hidden_dims: List[int], codebook_size: int, n_layers: int = 3,
                 n_cat_feats: int = 18, commitment_weight: float = 0.25, rqvae_weights_path: Optional[str] = None,
                 rqvae_codebook_normalize: bool = False, rqvae_sim_vq: bool = False) -> None:
        super().__init__()
        self.rq_vae = RqVae(input_dim=input_dim, embed_dim=output_dim, hidden_dims=hidden_dims,
                            codebook_size=codebook_size, codebook_kmeans_init=False,
                            codebook_normalize=rqvae_codebook_normalize, codebook_sim_vq=rqvae_sim_vq,
                            n_layers=n_layers, n_cat_features=n_cat_feats, commitment_weight=commitment_weight)
        if rqvae_weights_path is not None:
            self.rq_vae.load_pretrained(rqvae_weights_path)
        self.rq_vae.eval()
        self.codebook_size = codebook_size
        self.n_layers = n_layers
        self.reference_batching = True
        self.reset()

    def _get_hits(self, query: Tensor, key: Tensor) -> Tensor:
        return (key.unsqueeze(0) == query.unsqueeze(1)).all(dim=-1)

    def reset(self):
        self.cached_ids = None
        self._prefix_index = {}
        self._trie = None
        self._trie_index = None

    @property
    def sem_ids_dim(self):
        return self.n_layers + 1

    @torch.no_grad()
    @eval_mode
    def precompute_corpus_ids(self, movie_dataset, shard: bool = False, beam: int = 1,
                              resolve_collisions: bool = False) -> Tensor:
        """(N, L+1) corpus ids (semids.py:74-101). `shard=True` (a collective: every rank must call
        it) splits the quantization over the data-parallel ranks and all-gathers the ids.
        `beam` > 1 (this build's extension) encodes with the beam encoder (RqVae.get_semantic_id_beams): an item's
        id is its best of `beam` paths instead of the greedy one. `resolve_collisions=True` (needs beam >= 2)
        moves an item whose path another item already owns to its next-best path
        (modules.tokenizer.collisions.resolve, on the gathered paths: identical on every rank); the dedup column
        is computed afterwards as always. The defaults take the greedy code path unchanged."""
        if beam < 1 or (resolve_collisions and beam < 2):
            raise ValueError(f"precompute_corpus_ids: need beam >= 1, and beam >= 2 to resolve collisions (beam={beam})")
        dev = self.rq_vae.device
        n = len(movie_dataset)
        lo, hi = dp.shard_range(n, dp.rank(), dp.world()) if shard else (0, n)
        chunks = []
        for a in range(lo, hi, CORPUS_BATCH):
            batch = movie_dataset[list(range(a, min(hi, a + CORPUS_BATCH)))]
            x = batch.x.to(dev, non_blocking=True)
            if beam == 1:
                chunks.append(self.rq_vae.get_semantic_ids(x).sem_ids)
            else:
                chunks.append(self.rq_vae.get_semantic_id_beams(x, beam).sem_ids.reshape(x.shape[0], -1))
        ids = (torch.cat(chunks, 0) if chunks
               else torch.zeros((0, self.n_layers * beam), dtype=torch.int64, device=dev))
        if shard:
            ids = dp.all_gather_rows(ids, n)
        if beam > 1:
            paths = ids.view(n, beam, self.n_layers)
            if resolve_collisions:
                from modules.tokenizer import collisions
                ids = collisions.resolve(paths, self.codebook_size)[0]
            else:
                ids = paths[:, 0].contiguous()
        self.cached_ids = torch.cat([ids, dedup_rank(ids).unsqueeze(1)], 1)
        self._prefix_index = {}
        self._trie = None
        self._trie_index = None
        return self.cached_ids

    def _prefix_keys(self, P: int):
        if P not in self._prefix_index:
            cols = self.cached_ids[:, :P]
            base = int(self.cached_ids.max().item()) + 1
            self._prefix_index[P] = (torch.unique(_pack(cols, base)), base)
        return self._prefix_index[P]

    def prefix_table(self, P: int):
        """(keys, base): the sorted unique packed keys (`_pack` in base `base`) of the corpus ids' length-P
        prefixes — the table exists_prefix searches, for callers that search it on the device themselves
        (rqvae_hip.ops.beam_select). Cached per P until the corpus changes."""
        if self.cached_ids is None:
            raise Exception("No match can be found in empty cache.")
        return self._prefix_keys(P)

    @torch.no_grad()
    def prefix_trie(self) -> PrefixTrie:
        """The corpus ids (N, D) as a PrefixTrie, for callers that decode against it on the device
        (rqvae_hip.ops.beam_expand): only valid continuations of a prefix are ever scored. Built with torch ops on
        the device of `cached_ids` (CPU tensors work too); cached until the corpus changes."""
        if self.cached_ids is None:
            raise Exception("No match can be found in empty cache.")
        if self._trie is None:
            ids = self.cached_ids
            dev, D = ids.device, ids.shape[1]
            keys = [torch.zeros(1, dtype=torch.int64, device=dev)]
            base = 1
            for p in range(1, D + 1):
                k, base = self._prefix_keys(p)
                keys.append(k)
            tok, child_off = [None], []
            for p in range(1, D + 1):
                tok.append((keys[p] % base).to(torch.int32))
                parent = torch.searchsorted(keys[p - 1], torch.div(keys[p], base, rounding_mode="floor"))
                off = torch.zeros(keys[p - 1].numel() + 1, dtype=torch.int64, device=dev)
                off[1:] = torch.cumsum(torch.bincount(parent, minlength=keys[p - 1].numel()), 0)
                child_off.append(off.to(torch.int32))
            # a stable sort of the full rows' keys: the first row of every run is the lowest corpus index
            sk, order = torch.sort(_pack(ids, base), stable=True)
            first = torch.ones(sk.numel(), dtype=torch.bool, device=dev)
            first[1:] = sk[1:] != sk[:-1]
            self._trie = PrefixTrie(tok=tuple(tok), child_off=tuple(child_off), leaf_item=order[first], depth=D,
                                    base=base)
        return self._trie

    @torch.no_grad()
    def trie_index(self) -> TrieIndex:
        """prefix_trie()'s companion: every item's leaf, every leaf's ancestors and every node's leaf count. Built
        with torch ops on the device of `cached_ids` (CPU tensors work too); cached until the corpus changes."""
        trie = self.prefix_trie()
        if self._trie_index is None:
            ids, D, base = self.cached_ids, trie.depth, trie.base
            leaf_keys = self._prefix_keys(D)[0]
            item_leaf = torch.searchsorted(leaf_keys, _pack(ids, base)).to(torch.int32)
            anc, count = [], []
            for q in range(1, D + 1):
                keys = self._prefix_keys(q)[0]
                a = torch.searchsorted(keys, torch.div(leaf_keys, base ** (D - q), rounding_mode="floor"))
                anc.append(a.to(torch.int32))
                count.append(torch.bincount(a, minlength=keys.numel()).to(torch.int32))
            self._trie_index = TrieIndex(item_leaf=item_leaf, leaf_anc=tuple(anc), leaf_count=tuple(count))
        return self._trie_index

    @torch.no_grad()
    def blocked_nodes(self, items: Tensor) -> Tensor:
        """(D, B, H) int32 for `items` (B, H) int64 corpus indices, -1 (any entry outside [0, N)) as padding — the
        layout of SeqBatch.ids: slice q - 1 holds per user the BLOCKED level-q trie nodes, ascending and distinct,
        then INT32_MAX. A node is blocked iff every leaf below it is the row of a listed item (exclusion is by sem-ID
        row: an item whose row duplicates a listed one goes with it), so a constrained search that skips the blocked
        nodes of every level is exactly the search over the corpus without that user's rows
        (rqvae_hip.ops.beam_expand(blocked=...)). Device tensors: one HIP launch for all levels
        (rqvae_hip.ops.trie_blocked_nodes), no host read; CPU tensors: the same result with plain torch."""
        idx = self.trie_index()
        if items.dim() != 2:
            raise ValueError(f"blocked_nodes: items must be (B, H), got {tuple(items.shape)}")
        if items.is_cuda:
            from rqvae_hip import ops as hip_ops
            return hip_ops.trie_blocked_nodes(items.to(torch.int64).contiguous(), idx.item_leaf, idx.leaf_anc,
                                              idx.leaf_count)
        B, H = items.shape
        D, n = len(idx.leaf_anc), idx.item_leaf.numel()
        out = torch.full((D, B, H), _NO_NODE, dtype=torch.int32)
        if B == 0 or H == 0:
            return out
        ok = (items >= 0) & (items < n)
        leaf = torch.where(ok, idx.item_leaf[items.clamp(0, max(n - 1, 0))].long(), _NO_NODE).sort(dim=1).values
        dup = torch.zeros_like(ok)
        dup[:, 1:] = leaf[:, 1:] == leaf[:, :-1]
        leaf = torch.where(dup, _NO_NODE, leaf).sort(dim=1).values        # distinct leaves first, ascending
        live = leaf < _NO_NODE
        row = torch.arange(B).unsqueeze(1).expand(B, H)
        if not bool(live.any()):
            return out
        leaf = leaf.clamp_max(idx.leaf_anc[0].numel() - 1)                # padding reads the last leaf, masked by `live`
        for q in range(D):
            n_q = idx.leaf_count[q].numel()
            a = idx.leaf_anc[q].long()[leaf]                              # (B, H), non-decreasing over the live part
            # the user's listed leaves under every node, against the node's leaf count
            listed = torch.bincount((row * n_q + a)[live], minlength=B * n_q).view(B, n_q)
            head = live.clone()
            head[:, 1:] &= a[:, 1:] != a[:, :-1]                          # the first listed leaf of a node
            full = head & (listed[row, a] == idx.leaf_count[q].long()[a])
            out[q] = torch.where(full, a, _NO_NODE).sort(dim=1).values.to(torch.int32)
        return out

    def _group_table(self, what: str, name: str, table: Tensor, dtype):
        """The shared front of item_filter and item_bias: `table` checked — `dtype`, (N,) or (G, N) over the N corpus
        items, on the corpus ids' device — and as (G, N), then the trie index, G, N, the leaf count and the level
        sizes n_q."""
        idx = self.trie_index()
        N = idx.item_leaf.numel()
        if table.dtype != dtype or table.dim() not in (1, 2) or table.shape[-1] != N:
            raise ValueError(f"{what}: {name} must be {str(dtype)[6:]} (N,) or (G, N) with N = {N} corpus items, got "
                             f"{table.dtype} {tuple(table.shape)}")
        if table.device != idx.item_leaf.device:
            raise ValueError(f"{what}: {name} must live on the corpus ids' device {idx.item_leaf.device}, got "
                             f"{table.device}")
        if table.dim() == 1:
            table = table.unsqueeze(0)
        return table, idx, table.shape[0], N, idx.leaf_anc[0].numel(), [c.numel() for c in idx.leaf_count]

    @torch.no_grad()
    def item_filter(self, mask: Tensor) -> ItemFilter:
        """The ItemFilter of `mask`, bool (N,) or (G, N) over corpus indices: mask[g][i] says whether group g (a
        region, a category, a user) may be shown item i. A constrained search that keeps only the children whose bit
        is set at every level (rqvae_hip.ops.beam_expand(allowed=..., group=...)) is exactly the search over the
        sub-corpus of the allowed items, without a trie per filter. Filtering is by item, not by row: a row that
        several items share stays reachable while one of them is allowed and is reported under the lowest allowed
        index. Device tensors: two HIP launches for all levels (rqvae_hip.ops.trie_allowed_nodes), no host read; CPU
        tensors: the same tables with plain torch. Nothing is cached: build once, reuse across calls."""
        mask, idx, G, N, n_leaves, n_nodes = self._group_table("item_filter", "mask", mask, torch.bool)
        if mask.is_cuda:
            from rqvae_hip import ops as hip_ops
            bits, leaf_item = hip_ops.trie_allowed_nodes(mask.contiguous(), idx.item_leaf, idx.leaf_anc, n_nodes)
            return ItemFilter(bits=bits, leaf_item=leaf_item, groups=G)
        none = torch.iinfo(torch.int64).max
        leaf = idx.item_leaf.long().expand(G, N)
        lowest = torch.full((G, n_leaves), none, dtype=torch.int64)
        lowest.scatter_reduce_(1, leaf, torch.where(mask, torch.arange(N), none), "amin")
        leaf_ok = lowest != none
        shifts = torch.arange(32, dtype=torch.int64)
        bits = []
        for q, n_q in enumerate(n_nodes):
            W = (n_q + 31) // 32
            below = torch.zeros((G, W * 32), dtype=torch.int64)
            below.scatter_add_(1, idx.leaf_anc[q].long().expand(G, n_leaves), leaf_ok.long())   # allowed leaves below
            words = ((below > 0).view(G, W, 32).long() << shifts).sum(-1)                       # in [0, 2^32)
            bits.append(torch.where(words >= 2 ** 31, words - 2 ** 32, words).to(torch.int32))
        return ItemFilter(bits=tuple(bits), leaf_item=torch.where(leaf_ok, lowest, -1), groups=G)

    @torch.no_grad()
    def item_bias(self, bias: Tensor) -> ItemBias:
        """The ItemBias of `bias`, fp32 (N,) or (G, N) over corpus indices: bias[g][i] is what group g (a region, a
        campaign, a user) adds to item i's log-probability — a promotion boost, -alpha log popularity, a price prior,
        another ranker's score; -inf means "never show". Values are read cleaned: NaN and +inf as -inf (a bad value can
        only hide an item), -0.0 as +0.0. A constrained search that ranks every prefix by its log-probability plus its
        node's bound (rqvae_hip.ops.beam_expand_biased) spends its beams where the biased score can still be high, and
        ends on log p(item) + bias[g][item]. A row that several items share is reported under the item that attains the
        leaf's bound, the lowest index among equals. Device tensors: two HIP launches for all levels
        (rqvae_hip.ops.trie_bias_nodes), no host read; CPU tensors: the same tables, bit for bit, with plain torch.
        Nothing is cached: build once, reuse across calls."""
        bias, idx, G, N, n_leaves, n_nodes = self._group_table("item_bias", "bias", bias, torch.float32)
        if bias.is_cuda:
            from rqvae_hip import ops as hip_ops
            upper, leaf_item = hip_ops.trie_bias_nodes(bias.contiguous(), idx.item_leaf, idx.leaf_anc, n_nodes)
            return ItemBias(upper=upper, leaf_item=leaf_item, groups=G)
        ninf = float("-inf")
        clean = torch.where(bias.isnan() | (bias == float("inf")), ninf, bias)
        clean = torch.where(clean == 0, 0.0, clean)                       # -0.0 -> +0.0
        leaf = idx.item_leaf.long().expand(G, N)
        best = torch.full((G, n_leaves), ninf).scatter_reduce_(1, leaf, clean, "amax")
        none = torch.iinfo(torch.int64).max
        attains = (clean == best.gather(1, leaf)) & (clean > ninf)
        lowest = torch.full((G, n_leaves), none, dtype=torch.int64)
        lowest.scatter_reduce_(1, leaf, torch.where(attains, torch.arange(N), none), "amin")
        upper = tuple(torch.full((G, n_q), ninf).scatter_reduce_(1, idx.leaf_anc[q].long().expand(G, n_leaves), best, "amax")
                      for q, n_q in enumerate(n_nodes))
        return ItemBias(upper=upper, leaf_item=torch.where(lowest != none, lowest, -1), groups=G)

    @torch.no_grad()
    @eval_mode
    def exists_prefix(self, sem_id_prefix: Tensor) -> Tensor:
        if self.cached_ids is None:
            raise Exception("No match can be found in empty cache.")
        P = sem_id_prefix.shape[-1]
        keys, base = self._prefix_keys(P)
        q = sem_id_prefix.to(keys.device)
        in_range = ((q >= 0) & (q < base)).all(-1)
        qk = _pack(q.clamp(0, base - 1), base)
        pos = torch.searchsorted(keys, qk).clamp_max(keys.numel() - 1)
        out = (keys[pos] == qk) & in_range
        if self.reference_batching:
            checked = math.ceil(sem_id_prefix.shape[0] // BATCH_SIZE) * BATCH_SIZE
            out[checked:] = False
        return out.to(sem_id_prefix.device)

    def _tokenize_seq_batch_from_cached(self, ids: Tensor) -> Tensor:
        # id -1 indexes the last row (then masked by the caller), exactly like the reference (A-12)
        rows = self.cached_ids[ids.flatten()]
        return rows.reshape(ids.shape[0], -1)

    def cache_hit(self, ids_max: int) -> bool:
        """True when every id up to `ids_max` (host int) maps through the precomputed corpus cache: forward
        then launches only device lookups (no RQ-VAE pass, no host read), so it can be captured."""
        return self.cached_ids is not None and int(ids_max) < self.cached_ids.shape[0]

    @torch.no_grad()
    @eval_mode
    def forward(self, batch: SeqBatch, ids_max: Optional[int] = None) -> TokenizedSeqBatch:
        """`ids_max` (this build's extension): the batch's largest item id when the caller knows it on the
        host (a CPU-side loader), so the cache check needs no device read (a sync every step)."""
        B, N = batch.ids.shape
        top = batch.ids.max() if ids_max is None else ids_max
        if self.cached_ids is None or top >= self.cached_ids.shape[0]:
            sem_ids = self.rq_vae.get_semantic_ids(batch.x).sem_ids
            D = sem_ids.shape[-1]
            seq_mask, sem_ids_fut = None, None
        else:
            D = self.cached_ids.shape[1]
            sem_ids = self._tokenize_seq_batch_from_cached(batch.ids)
            seq_mask = batch.seq_mask.repeat_interleave(D, dim=1)
            sem_ids = sem_ids.masked_fill(~seq_mask, -1)
            sem_ids_fut = self._tokenize_seq_batch_from_cached(batch.ids_fut)
        token_type_ids = torch.arange(D, device=sem_ids.device).repeat(B, N)
        token_type_ids_fut = torch.arange(D, device=sem_ids.device).repeat(B, 1)
        return TokenizedSeqBatch(user_ids=batch.user_ids, sem_ids=sem_ids, sem_ids_fut=sem_ids_fut, seq_mask=seq_mask,
                                 token_type_ids=token_type_ids, token_type_ids_fut=token_type_ids_fut)
