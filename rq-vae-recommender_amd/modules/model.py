"""Generative-retrieval encoder-decoder — drop-in for reference modules/model.py
(ModelOutput :30-33, GenerationOutput :36-38, EncoderDecoderRetrievalModel :41-282; same
constructor, parameter names, forward/generation contract).

Forward (training) path, jagged mode (the only working mode in the reference, SURVEY A-9):
  user token + (wpe + sem-ID embeddings) -> padded (B, 1+N, E) context, bos + (fut sem-ID +
  tte) -> (B, L+2, E) future; both converted to NJTs by the HIP gather kernel (ops.jagged);
  RMSNorm -> Dropout(0.5) -> in_proj{_context}; TransformerEncoderDecoder on NJT values with the
  HIP varlen attention kernels; out_proj -> logits (B*(L+1), K) -> CE(ignore_index=-1) summed
  over the L+1 positions and averaged over B; loss_d = per-position mean.
The module-level Dropout(p=0.5) is hard-coded as in the reference (:67).
"""
import contextlib
from typing import NamedTuple

import torch
from torch import nn
from torch import Tensor
from torch.nn import functional as F

from data.schemas import TokenizedSeqBatch
from modules.linear import Linear
from modules.embedding.id_embedder import Embedding, SemIdEmbedder, UserIdEmbedder
from modules.normalize import RMSNorm
from modules.tokenizer.semids import ItemBias
from modules.transformer.model import TransformerEncoderDecoder
from modules.utils import eval_mode, maybe_repeat_interleave, reset_encoder_cache
from ops.jagged import Jagged, jagged_to_flattened_tensor, jagged_to_padded_tensor, padded_to_jagged, row_counts
from rqvae_hip import gemm_tuning
from rqvae_hip import ops as hip_ops

# The fused forms below are the product path; False selects the reference's torch composition of the same
# op (tests / A-B probes set these module attributes; nothing reads the environment):
_BATCH_SUM = True   # False: torch's broadcast add / repeat (and their reduction backward) in the prologue
_FUSED_CE = True    # False: the loss head as torch's slice + cross_entropy + means
_FUSED_PROLOGUE = True   # False: the input embeddings as gathers / adds / cats + padded -> jagged (the composition)

# As the reference (modules/model.py:27): fp32 matmuls at 'high' precision (split-bf16 GEMM on
# gfx950, rqvae_hip.ops.gemm_bf16x3); 'highest' restores the exact-fp32 library path.
torch.set_float32_matmul_precision('high')


class ModelOutput(NamedTuple):
    loss: Tensor
    logits: Tensor
    loss_d: Tensor


class GenerationOutput(NamedTuple):
    sem_ids: Tensor
    log_probas: Tensor


class Recommendation(NamedTuple):
    item_ids: Tensor     # (B, k) int64 corpus indices, -1 for dead beams
    sem_ids: Tensor      # (B, k, D)
    log_probas: Tensor   # (B, k)


class RankedItems(NamedTuple):
    """recommend(item_bias=...): the rows are ordered by `scores`, descending."""
    item_ids: Tensor     # (B, k) int64 corpus indices, -1 for dead beams
    sem_ids: Tensor      # (B, k, D)
    log_probas: Tensor   # (B, k) fp32: the raw model score log p(item | user), what score_items reproduces
    scores: Tensor       # (B, k) fp32: log_probas + bias[group][item] (one fp32 add); log_probas for an unbiased user


class SampledItems(NamedTuple):
    item_ids: Tensor     # (B, k) int64 corpus indices, -1 for dead rows
    sem_ids: Tensor      # (B, k, D)
    log_probas: Tensor   # (B, k) fp32: log-probability under the renormalised trie distribution, -inf for dead rows
    perturbed: Tensor    # (B, k) fp32: the Gumbel-perturbed scores the rows are ordered by, descending; [:, 0] == 0


class Scores(NamedTuple):
    log_probas: Tensor   # (B, C) fp32, -inf for padding and for candidates the model cannot generate
    rank: Tensor         # (B, C) int32: each candidate's place among its user's, a permutation of 0..C-1


class _TrieSearch(NamedTuple):
    """A trie search's per-call tables (EncoderDecoderRetrievalModel._trie_search)."""
    trie: object
    blocked: Tensor   # (D, B, H) int32 blocked nodes of every level, or None
    table: object     # the call's group table: an ItemFilter, an ItemBias or None
    group: Tensor     # (B,) int32 with a table: every user's row of it; else None

    @property
    def biased(self) -> bool:
        return isinstance(self.table, ItemBias)

    @property
    def expand(self):
        """The deterministic step's op: hip_ops.beam_expand_biased under an ItemBias, else hip_ops.beam_expand (the
        sampled step, hip_ops.beam_expand_sampled, takes beam_expand's keywords and no bias)."""
        return hip_ops.beam_expand_biased if self.biased else hip_ops.beam_expand

    def level(self, i: int) -> dict:
        """Step i's trie and table keywords of `expand`."""
        lvl = dict(child_off=self.trie.child_off[i], tok=self.trie.tok[i + 1],
                   blocked=None if self.blocked is None else self.blocked[i])
        if self.biased:
            return dict(lvl, bias=self.table.upper[i], bias_group=self.group)
        return dict(lvl, allowed=None if self.table is None else self.table.bits[i], group=self.group)


class EncoderDecoderRetrievalModel(nn.Module):
    def __init__(self, embedding_dim, attn_dim, dropout, num_heads, n_layers, num_embeddings, sem_id_dim,
                 inference_verifier_fn, max_pos=2048, jagged_mode: bool = True) -> None:
        super().__init__()
        if not jagged_mode:
            raise NotImplementedError("jagged_mode=False is broken in the reference (SURVEY A-9); "
                                      "only the jagged path is provided")
        self.jagged_mode = jagged_mode
        self.num_embeddings = num_embeddings
        self.sem_id_dim = sem_id_dim
        self.attn_dim = attn_dim
        self.inference_verifier_fn = inference_verifier_fn
        # optional: an object with prefix_table(P) and reference_batching (the SemanticIdTokenizer); fused
        # generation then verifies prefixes inside its select kernel instead of calling inference_verifier_fn, and
        # constrained generation / recommend walk its prefix_trie()
        self.inference_prefix_index = None
        self.enable_generation = False

        self.bos_emb = nn.Parameter(torch.rand(embedding_dim))
        self.norm = RMSNorm(embedding_dim)
        self.norm_cxt = RMSNorm(embedding_dim)
        self.do = nn.Dropout(p=0.5)
        self.sem_id_embedder = SemIdEmbedder(num_embeddings=num_embeddings, sem_ids_dim=sem_id_dim,
                                             embeddings_dim=embedding_dim)
        self.user_id_embedder = UserIdEmbedder(2000, embedding_dim)
        self.wpe = Embedding(num_embeddings=max_pos, embedding_dim=embedding_dim)
        self.tte = Embedding(num_embeddings=sem_id_dim, embedding_dim=embedding_dim)
        self.tte_fut = Embedding(num_embeddings=sem_id_dim, embedding_dim=embedding_dim)  # unused (reference)
        self.transformer = TransformerEncoderDecoder(d_in=attn_dim, d_out=attn_dim, dropout=dropout,
                                                     num_heads=num_heads, encoder_layers=n_layers // 2,
                                                     decoder_layers=n_layers // 2)
        self.in_proj = Linear(embedding_dim, attn_dim, bias=False)
        self.in_proj_context = Linear(embedding_dim, attn_dim, bias=False)
        self.out_proj = Linear(attn_dim, num_embeddings, bias=False)

    def __setattr__(self, name, value):
        if name == "inference_prefix_index":   # held by reference: the tokenizer must not become a submodule
            object.__setattr__(self, name, value)
        else:
            super().__setattr__(name, value)

    @staticmethod
    def context_rows(batch: TokenizedSeqBatch, bucket=None) -> int:
        """Allocated rows of the jagged context: valid tokens (user token + sequence) rounded up to
        `bucket`. Host-known counts (ops.jagged.register_row_counts) avoid the device sync."""
        B = batch.seq_mask.shape[0]
        host = row_counts(batch.seq_mask)
        total = host[0] + B if host is not None and host[3] == B else int(batch.seq_mask.sum()) + B
        return total if not bucket else (total + bucket - 1) // bucket * bucket

    def _prologue_fused(self, batch: TokenizedSeqBatch, alloc: int):
        """Context / future jagged inputs in one HIP op (hip_ops.decoder_prologue), or None where it does not
        apply (generation: no future tokens)."""
        se, ue = self.sem_id_embedder, self.user_id_embedder
        args = (ue.emb.weight, se.emb.weight, self.wpe.weight, self.tte.weight, self.bos_emb, batch.user_ids,
                batch.sem_ids, batch.token_type_ids, batch.seq_mask, batch.sem_ids_fut, batch.token_type_ids_fut)
        if not (_FUSED_PROLOGUE and hip_ops.decoder_prologue_supported(*args) and
                all(e.max_norm is None for e in (se.emb, ue.emb, self.wpe, self.tte)) and
                all(e.padding_idx is None for e in (ue.emb, self.wpe, self.tte))):
            return None
        B, N = batch.sem_ids.shape
        nf = batch.sem_ids_fut.shape[1] + 1
        ctx_v, ctx_off, fut_v, fut_off = hip_ops.decoder_prologue(*args, ue.num_buckets, se.num_embeddings,
                                                                   se.padding_idx, alloc)
        return Jagged(ctx_v, ctx_off, N + 1, 0, None), Jagged(fut_v, fut_off, nf, nf, B * nf)

    def _predict(self, batch: TokenizedSeqBatch):
        bucket = gemm_tuning.ROW_BUCKET if gemm_tuning.is_enabled() else None
        fused = self._prologue_fused(batch, self.context_rows(batch, bucket))
        if fused is not None:
            ctx_j, fut_j = fused
            transformer_context = ctx_j.with_values(self.in_proj_context(self.norm.forward_dropout(ctx_j.values(),
                                                                                                   self.do)))
            transformer_input = fut_j.with_values(self.in_proj(self.norm_cxt.forward_dropout(fut_j.values(), self.do)))
            return self.transformer(x=transformer_input, context=transformer_context, padding_mask=batch.seq_mask,
                                    jagged=True)
        user_emb = self.user_id_embedder(batch.user_ids)                  # (B, 1, E)
        sem = self.sem_id_embedder(batch)
        seq_emb, fut_emb = sem.seq, sem.fut                               # (B, N, E), (B, L+1, E)
        B, N, _ = seq_emb.shape
        pos = self.wpe(torch.arange(N, device=seq_emb.device)).unsqueeze(0)
        if _BATCH_SUM:   # the broadcast parameters' batch-sum gradients on one fixed-order HIP launch each
            ctx = torch.cat([user_emb, hip_ops.batch_add(seq_emb, pos)], dim=1)          # (B, 1+N, E)
            fut = hip_ops.batch_repeat(self.bos_emb.view(1, -1), B)
        else:
            ctx = torch.cat([user_emb, pos + seq_emb], dim=1)
            fut = self.bos_emb.repeat(B, 1, 1)
        if fut_emb is not None:
            fut = torch.cat([fut, fut_emb + self.tte(batch.token_type_ids_fut)], dim=1)
        ctx_lengths = batch.seq_mask.sum(axis=1) + 1
        # the context's valid row total is data-dependent; a CPU-side loader registers it with the
        # mask (no device sync). The values buffer is allocated at the total rounded up to the GEMM
        # row bucket (bounded GEMM shapes; rqvae_hip.gemm_tuning); the gather and attention kernels
        # keep the tail rows zero on the device, and attention is launched over the padded width,
        # so nothing in the step depends on the exact total on the host: a step captured for one
        # bucket (rqvae_hip.graph.GraphedSteps) replays for every batch of that bucket.
        bucket = gemm_tuning.ROW_BUCKET if gemm_tuning.is_enabled() else None
        alloc = self.context_rows(batch, bucket)
        Nc = ctx.shape[1]
        ctx_j = padded_to_jagged(ctx.contiguous(), ctx_lengths, Nc, alloc_rows=alloc, known_max=Nc)
        nf = fut.shape[1]                                                                # fixed length: no sync
        fut_lengths = torch.full((B,), nf, device=fut.device, dtype=torch.int64)
        fut_j = padded_to_jagged(fut.contiguous(), fut_lengths, nf, total=B * nf, known_max=nf)
        transformer_context = ctx_j.with_values(self.in_proj_context(self.norm.forward_dropout(ctx_j.values(), self.do)))
        transformer_input = fut_j.with_values(self.in_proj(self.norm_cxt.forward_dropout(fut_j.values(), self.do)))
        return self.transformer(x=transformer_input, context=transformer_context, padding_mask=batch.seq_mask,
                                jagged=True)

    def _context_inputs(self, batch: TokenizedSeqBatch) -> Jagged:
        """The encoder's jagged input alone (_predict's context half, the torch composition; eval: no dropout)."""
        user_emb = self.user_id_embedder(batch.user_ids)                  # (B, 1, E)
        seq_emb = self.sem_id_embedder(batch._replace(sem_ids_fut=None, token_type_ids_fut=None)).seq
        N = seq_emb.shape[1]
        pos = self.wpe(torch.arange(N, device=seq_emb.device)).unsqueeze(0)
        if _BATCH_SUM:
            ctx = torch.cat([user_emb, hip_ops.batch_add(seq_emb, pos)], dim=1)
        else:
            ctx = torch.cat([user_emb, pos + seq_emb], dim=1)
        bucket = gemm_tuning.ROW_BUCKET if gemm_tuning.is_enabled() else None
        ctx_j = padded_to_jagged(ctx.contiguous(), batch.seq_mask.sum(axis=1) + 1, N + 1,
                                 alloc_rows=self.context_rows(batch, bucket), known_max=N + 1)
        return ctx_j.with_values(self.in_proj_context(self.norm.forward_dropout(ctx_j.values(), self.do)))

    def _gemm_weights(self):
        return [m.weight for m in self.modules() if isinstance(m, nn.Linear)]

    def _gemm_weight_stacks(self):
        """Weights the forward multiplies as one concatenated matrix (the decoder's hoisted K/V)."""
        return [st for st in (getattr(m, "hoisted_kv_weights", lambda: None)() for m in self.modules()) if st]

    def forward(self, batch: TokenizedSeqBatch) -> ModelOutput:
        B = batch.seq_mask.shape[0]
        # every Linear weight split once per forward in a few launches (no-op at 'highest')
        with hip_ops.weight_split_scope(self._gemm_weights(), self._gemm_weight_stacks()):
            return self._forward(batch, B)

    def _forward(self, batch: TokenizedSeqBatch, B: int) -> ModelOutput:
        trnsf_out = self._predict(batch)
        if self.training or not self.enable_generation:
            predict_out = self.out_proj(jagged_to_flattened_tensor(trnsf_out))
            target = batch.sem_ids_fut
            if _FUSED_CE and hip_ops.ce_loss_supported(predict_out, target, B):
                # the whole loss head (slice, cross-entropy, both means) in three HIP launches
                loss, loss_d, logits = hip_ops.cross_entropy_loss(predict_out, target, B)
                if not self.training:
                    self.transformer.cached_enc_output = None
                return ModelOutput(loss=loss, logits=logits, loss_d=loss_d)
            # sem_ids_fut is fixed length, so the jagged values reshape to (B, L+2, K)
            logits = predict_out.view(B, -1, self.num_embeddings)[:, :-1, :].flatten(end_dim=1)
            target = batch.sem_ids_fut.flatten(end_dim=1)
            unred_loss = F.cross_entropy(logits, target, reduction="none", ignore_index=-1).view(B, -1)
            loss = unred_loss.sum(axis=1).mean()
            if not self.training:
                self.transformer.cached_enc_output = None
            return ModelOutput(loss=loss, logits=logits, loss_d=unred_loss.mean(axis=0))
        last = jagged_to_flattened_tensor(trnsf_out).contiguous().view(B, -1, self.attn_dim)[:, -1, :]
        return ModelOutput(loss=None, logits=self.out_proj(last), loss_d=None)

    @eval_mode
    @reset_encoder_cache
    @torch.no_grad()
    def generate_next_sem_id(self, batch: TokenizedSeqBatch, temperature: int = 1, top_k: bool = True, *,
                             fused: bool = False, sample: bool = True,
                             incremental: bool = False, constrained: bool = False,
                             exclude_items: Tensor = None, beams: int = 32, item_filter=None,
                             filter_group: Tensor = None) -> GenerationOutput:
        """Beam-style decoding of the next item's L+1 sem-ID tokens (reference :149-245): per step
        sample 200 candidates per beam from softmax(logits / T), drop prefixes the verifier
        rejects (-10000), keep the top 32 cumulative log-probabilities. The encoder output is
        computed once and repeated per beam with the HIP jagged kernels (jagged -> padded,
        repeat_interleave, padded -> jagged), as the reference does with torch ops.
        fused=True: each step's softmax, sampling, verification, top-k and parent gather on two HIP
        launches (_generate_sampled); sample=False then takes the most probable candidates instead of a draw.
        incremental=True (needs fused=True): the same loop over a BeamDecodeState — the context's cross-attention
        K / V projected once for the B users and only each beam's newest token run through the decoder
        (_step_logits).
        constrained=True (needs fused=True, an explicit sample=False and `inference_prefix_index`): the beams walk
        the corpus' prefix trie (_generate_constrained), one hip_ops.beam_expand launch per step; with or without
        incremental. Deterministic (no generator draw), every valid continuation is scored (not 200 of them), every
        returned beam is a corpus item or dead (ids -1, log-probability -inf) when a user has fewer valid beams than
        k. `reference_batching` does not apply and is not consulted.
        exclude_items (needs constrained=True): (B, H <= 1024) int64 corpus indices, -1 as padding (the layout of
        SeqBatch.ids) — the search runs over the corpus without each user's listed rows (an item whose sem-ID row
        duplicates a listed one goes with it): the tokenizer's blocked_nodes mask, built by one launch per call, is
        applied by beam_expand at every level, so no beam is spent on a prefix that only leads to listed items.
        beams (needs constrained=True and top_k=True): the search's width, 1..1024 beams per user instead of 32 — the
        returned tensors are (B, beams, L+1) / (B, beams); past 32 beams at V = 256 the steps run the wide expand
        kernel (hip_ops.beam_expand(wide=None)), at 32 they are the launches they were.
        item_filter (needs constrained=True): a catalogue filter — the search runs over the sub-corpus of the ALLOWED
        items ("only what is in stock"), without a trie per filter. An ItemFilter (the tokenizer's item_filter(mask),
        built once and reused) or a bool mask (N,) / (G, N) over corpus indices, turned into one per call. filter_group
        (B,) integer: each user's group (row of the mask); -1 leaves a user unfiltered; None is group 0 for everyone,
        which needs a one-group filter. Step i's beam_expand keeps only the children whose bit is set in
        item_filter.bits[i]; it composes with exclude_items (a candidate passes both), beams and incremental."""
        if not 1 <= beams <= hip_ops.BEAM_WIDE_MAX:
            raise ValueError(f"generate_next_sem_id: need 1 <= beams <= {hip_ops.BEAM_WIDE_MAX}, got {beams}")
        if beams != 32 and not (constrained and top_k):
            raise ValueError("generate_next_sem_id: beams is the width of the constrained search; it requires "
                             "constrained=True and top_k=True")
        if incremental and not fused:
            raise ValueError("generate_next_sem_id: incremental=True requires fused=True")
        if exclude_items is not None and not constrained:
            raise ValueError("generate_next_sem_id: exclude_items requires constrained=True")
        if (item_filter is not None or filter_group is not None) and not constrained:
            raise ValueError("generate_next_sem_id: item_filter / filter_group require constrained=True")
        if constrained:
            if not fused:
                raise ValueError("generate_next_sem_id: constrained=True requires fused=True")
            if sample:
                raise ValueError("generate_next_sem_id: constrained=True is deterministic; pass sample=False")
            self._constrained_trie("generate_next_sem_id")
        assert self.enable_generation, "Model generation is not enabled"
        if constrained:
            search = self._trie_search("generate_next_sem_id", batch, exclude_items, item_filter, filter_group)
            generated, log_probas, _, _ = self._generate_constrained(batch, temperature, beams if top_k else 1,
                                                                     incremental, search)
            return GenerationOutput(sem_ids=generated.squeeze(), log_probas=log_probas.squeeze())
        if fused:
            return self._generate_sampled(batch, temperature, top_k, sample, incremental)
        B = batch.sem_ids.shape[0]
        generated, log_probas = None, 0
        k = 32 if top_k else 1
        n_cand = 200 if top_k else 1
        step = _ForwardSteps(self, batch)
        for i in range(self.sem_id_dim):
            logits = step() if generated is None else step(generated)
            probas = F.softmax(logits / temperature, dim=-1)
            samples_b = torch.multinomial(probas, num_samples=n_cand)
            if generated is None:
                valid = self.inference_verifier_fn(samples_b.unsqueeze(-1))
            else:
                prefix = torch.cat([generated.flatten(0, 1).unsqueeze(1).repeat_interleave(n_cand, axis=1),
                                    samples_b.unsqueeze(-1)], axis=-1)
                valid = self.inference_verifier_fn(prefix).reshape(B, -1)
            sampled_lp = torch.log(torch.gather(probas, 1, samples_b)).reshape(B, -1)
            samples = samples_b.reshape(B, -1)
            sorted_lp, sorted_idx = (-10000 * (~valid) + sampled_lp +
                                     maybe_repeat_interleave(log_probas, n_cand, dim=1)).sort(-1, descending=True)
            top_lp, top_idx = sorted_lp[:, :k], sorted_idx[:, :k]
            top_samples = torch.gather(samples, 1, top_idx)
            if generated is not None:
                parent = torch.gather(generated, 1, (top_idx // n_cand).unsqueeze(2).expand(-1, -1, i))
                generated = torch.cat([parent, top_samples.unsqueeze(-1)], axis=-1).detach().clone()
            else:
                generated = top_samples.unsqueeze(-1)
            log_probas = top_lp.detach().clone()
        return GenerationOutput(sem_ids=generated.squeeze(), log_probas=log_probas.squeeze())

    def _constrained_trie(self, what: str, items: bool = False):
        """The tokenizer's prefix trie, deep enough for the search; items: its leaves must be the corpus items."""
        index = getattr(self, "inference_prefix_index", None)
        if index is None:
            raise ValueError(f"{what}: constrained decoding requires inference_prefix_index (the tokenizer)")
        trie = index.prefix_trie()
        if trie.depth < self.sem_id_dim:
            raise ValueError(f"{what}: the corpus trie has depth {trie.depth} < sem_id_dim = {self.sem_id_dim}")
        if items and trie.depth != self.sem_id_dim:
            raise ValueError(f"{what}: the corpus trie has depth {trie.depth}, the model generates {self.sem_id_dim} "
                             "tokens; items are the leaves of the full depth")
        return trie

    def _trie_search(self, what: str, batch: TokenizedSeqBatch, exclude_items, item_filter, filter_group,
                     item_bias=None, bias_group=None) -> _TrieSearch:
        """The per-call tables of a search over the trie, and the one place a public call's exclude_items, item_filter /
        filter_group and item_bias / bias_group are validated, errors under the caller's name `what`: the trie, the
        users' blocked nodes of every level (exclude_items (B, H); the tokenizer's blocked_nodes, one launch for the
        whole call) and the call's group table — the catalogue filter or the score bias, never both (_group_table).
        _TrieSearch.level(i) hands step i its slices."""
        trie = self._constrained_trie(what)
        index, B, dev = self.inference_prefix_index, batch.sem_ids.shape[0], batch.sem_ids.device
        if item_filter is not None and item_bias is not None:
            raise ValueError(f"{what}: item_filter and item_bias cannot be combined; write the filter into the bias "
                             "as -inf (a {0, -inf} table is a hard filter)")
        table, group = self._group_table(what, "item_filter", "filter_group", "unfiltered", item_filter, filter_group,
                                         B, dev)
        bias = self._group_table(what, "item_bias", "bias_group", "unbiased", item_bias, bias_group, B, dev)
        if bias[0] is not None:
            table, group = bias
        blocked = None
        if exclude_items is not None:
            if exclude_items.dim() != 2 or exclude_items.shape[0] != B:
                raise ValueError(f"{what}: exclude_items must be (B, H) with B = {B} rows, got "
                                 f"{tuple(exclude_items.shape)}")
            blocked = index.blocked_nodes(exclude_items)
        return _TrieSearch(trie, blocked, table, group)

    def _group_table(self, what: str, arg: str, group_arg: str, off: str, table, group, B: int, device):
        """(table, group (B,) int32 on the device) of a call's table argument `arg` and group argument `group_arg`, or
        (None, None) without a table. A raw tensor becomes a table through the tokenizer's method of `arg`'s name
        (item_filter / item_bias; built per call); group None is row 0 for everyone, which needs a one-group table (-1
        leaves a user `off`); the groups are converted on the device, nothing is read back."""
        if table is None:
            if group is not None:
                raise ValueError(f"{what}: {group_arg} without {arg}")
            return None, None
        if isinstance(table, Tensor):
            table = getattr(self.inference_prefix_index, arg)(table)
        if group is None:
            if table.groups != 1:
                raise ValueError(f"{what}: {arg} has {table.groups} groups; {group_arg} (B,) must say which one every "
                                 f"user reads (-1: {off})")
            return table, torch.zeros(B, dtype=torch.int32, device=device)
        if group.dim() != 1 or group.shape[0] != B or group.dtype.is_floating_point or group.dtype == torch.bool:
            raise ValueError(f"{what}: {group_arg} must be (B,) integer with B = {B}, got {group.dtype} "
                             f"{tuple(group.shape)}")
        return table, group.to(device=device, dtype=torch.int32).contiguous()

    @staticmethod
    def _leaf_items(search: _TrieSearch, node: Tensor) -> Tensor:
        """The corpus index of every leaf node (B, k), -1 for dead rows: the trie's lowest index for a user outside
        the search's table (no table, or a group outside it), else the table's own leaf item of the user's group — an
        ItemFilter's lowest ALLOWED index, an ItemBias' item that attains the leaf's bound."""
        node = node.long()
        at = node.clamp_min(0)
        items = search.trie.leaf_item[at]
        table = search.table
        if table is not None:
            g = search.group.long().unsqueeze(1)
            inside = (g >= 0) & (g < table.groups)
            if table.groups > 0:
                items = torch.where(inside, table.leaf_item[g.clamp(0, table.groups - 1), at], items)
        return torch.where(node >= 0, items, -1)

    @eval_mode
    @reset_encoder_cache
    @torch.no_grad()
    def recommend(self, batch: TokenizedSeqBatch, k: int = 10, temperature: int = 1,
                  incremental: bool = True, exclude_items: Tensor = None, beams: int = 32, item_filter=None,
                  filter_group: Tensor = None, item_bias=None, bias_group: Tensor = None):
        """The k <= beams most probable corpus items for every user: the constrained beam search (`beams` wide, 32
        by default and up to 1024; sample=False; generate_next_sem_id(constrained=True, beams=beams)) with each kept
        beam mapped back to its corpus index through the trie's leaves. A user with fewer than k valid beams gets
        item id -1 (sem ids -1, log-probability -inf) in the remaining places. exclude_items (B, H) int64, -1 as padding: corpus items (and
        the items sharing their sem-ID rows) that are never returned — the k best of the REMAINING corpus, see
        generate_next_sem_id. item_filter / filter_group: a catalogue filter, see generate_next_sem_id — the k best of the
        ALLOWED items of each user's group; every returned id is an allowed item (a row that several items share is
        reported under its lowest allowed index), never a disallowed one.
        item_bias / bias_group: rank by the model's score PLUS a per-item adjustment (promotion boosts, popularity
        de-biasing, recency or price priors, another ranker's score) — an ItemBias (the tokenizer's item_bias(bias),
        built once and reused) or a raw fp32 tensor (N,) / (G, N) over corpus indices, turned into one per call; -inf
        never shows an item. bias_group (B,) integer: each user's row; -1 leaves a user unbiased; None is row 0 for
        everyone, which needs a one-group bias. The search itself is biased (hip_ops.beam_expand_biased): every prefix
        is ranked by its log-probability plus the largest adjustment of an item below its node, an optimistic estimate
        of the best final score there, so the beams go where the adjusted score can still be high — an item whose boost
        puts it first is found although its first token is unlikely, which over-fetching and re-ranking cannot promise;
        with `beams` at the width of the trie the result is exhaustive and exact. The result is then a RankedItems:
        rows ordered by `scores` = log p(item | user) + bias[group][item] descending, `log_probas` the raw model score
        (score_items' value), item ids from the ItemBias' leaves for biased users (a row several items share is
        reported under its highest-bias item). Composes with beams, incremental and exclude_items; together with
        item_filter it raises (write the filter into the bias as -inf). Without item_bias the call and its
        Recommendation are what they were."""
        if not 1 <= k <= beams <= hip_ops.BEAM_WIDE_MAX:
            raise ValueError(f"recommend: need 1 <= k <= {beams} beams <= {hip_ops.BEAM_WIDE_MAX}, got k = {k}")
        self._constrained_trie("recommend", items=True)
        assert self.enable_generation, "Model generation is not enabled"
        search = self._trie_search("recommend", batch, exclude_items, item_filter, filter_group, item_bias, bias_group)
        generated, log_probas, node, scores = self._generate_constrained(batch, temperature, beams, incremental, search)
        items = self._leaf_items(search, node[:, :k])
        if search.biased:
            return RankedItems(item_ids=items, sem_ids=generated[:, :k], log_probas=log_probas[:, :k],
                               scores=scores[:, :k])
        return Recommendation(item_ids=items, sem_ids=generated[:, :k], log_probas=log_probas[:, :k])

    @eval_mode
    @reset_encoder_cache
    @torch.no_grad()
    def sample_items(self, batch: TokenizedSeqBatch, k: int = 10, temperature: int = 1, incremental: bool = True,
                     exclude_items: Tensor = None, generator: torch.Generator = None, item_filter=None,
                     filter_group: Tensor = None) -> SampledItems:
        """k distinct corpus items per user, drawn without replacement in proportion to the model's own distribution
        over the corpus: stochastic beam search (Kool, van Hoof and Welling 2019) over the prefix trie, k beams wide,
        one hip_ops.beam_expand_sampled launch per token. The distribution is the trie's: at every node the model's
        softmax(logits / temperature) renormalised over the node's children, so the items' probabilities sum to 1.
        Rows are ordered by `perturbed` descending: row 0 is one exact draw, the first r rows a draw of r items
        without replacement. A user with fewer than k distinct rows left gets dead rows at the end (item id -1, sem
        ids -1, -inf). `log_probas` is log of that renormalised probability — NOT the full-V score recommend()
        returns; score_items(batch, item_ids) gives the raw model score. `perturbed[:, 0]` is exactly 0 (the root's
        perturbed score is pinned there; the order does not depend on it). exclude_items (B, H) int64, -1 as padding,
        as recommend: the draw is from the corpus minus the listed rows (and the items sharing them). item_filter /
        filter_group, as recommend: the draw is from the allowed items of each user's group, the distribution
        renormalised over the children that still lead to one.
        The draws, part of the contract: at step i, on that step's logits (B, V) / (B * k, V),
        exactly one torch.empty_like(logits).exponential_(generator=generator), steps in order, nothing else;
        generator=None is the device's default generator. Needs k * num_embeddings <= 8192."""
        limit = hip_ops.BEAM_MAX_N // self.num_embeddings
        if not 1 <= k <= limit:
            raise ValueError(f"sample_items: need 1 <= k and k * num_embeddings <= {hip_ops.BEAM_MAX_N}, that is "
                             f"k <= {limit} at num_embeddings = {self.num_embeddings}; got k = {k}")
        self._constrained_trie("sample_items", items=True)
        assert self.enable_generation, "Model generation is not enabled"
        B = batch.sem_ids.shape[0]
        search = self._trie_search("sample_items", batch, exclude_items, item_filter, filter_group)
        generated, phi, g, parent, node = None, None, None, None, None
        with self._step_logits(batch, incremental) as step:
            for i in range(self.sem_id_dim):
                logits = (step() if generated is None else step(generated.clamp_min(0), parent)).contiguous()
                noise = torch.empty_like(logits).exponential_(generator=generator)
                generated, phi, g, parent, node = hip_ops.beam_expand_sampled(
                    logits, k, batch=B, noise=noise, node=node, parents=generated, parent_phi=phi, parent_g=g,
                    temperature=temperature, **search.level(i))
        items = self._leaf_items(search, node)
        return SampledItems(item_ids=items, sem_ids=generated, log_probas=phi, perturbed=g)

    @eval_mode
    @reset_encoder_cache
    @torch.no_grad()
    def score_sem_ids(self, batch: TokenizedSeqBatch, sem_ids: Tensor, temperature: int = 1,
                      incremental: bool = True) -> Scores:
        """log p(sem-ID tuple | user) for C tuples per user that the caller names: sem_ids (B, C, D) int64 with
        D = sem_id_dim and 1 <= C <= 1024. A tuple whose first token is negative is padding (log-probability -inf,
        ranked last); any other tuple is scored as it stands — it need not be a corpus row, nothing consults the
        trie — and one naming a token outside [0, num_embeddings), a class the model cannot generate, gets -inf.
        The walk is teacher-forced: step i's logits for every candidate's own prefix, one hip_ops.score_paths launch
        per step that adds the log-softmax at the candidate's token. Scores are the model's full-V softmax, formed as
        beam_expand forms them, so a tuple that recommend() / generate_next_sem_id(constrained=True) returns scores
        what it was returned with. `rank` is each tuple's place in its user's (score descending, index ascending)
        order, a permutation of 0..C-1. No generator draw, no host read, no beam search.
        incremental=True: one BeamDecodeState — the encoder and the cross-attention K / V once per user, then only the
        newest token of every candidate (every candidate its own ancestor); incremental=False: full forwards over
        _beams_batch batches (the independent path; _step_logits holds both)."""
        assert self.enable_generation, "Model generation is not enabled"
        if sem_ids.dim() != 3 or sem_ids.dtype != torch.int64:
            raise ValueError(f"score_sem_ids: sem_ids must be (B, C, D) int64, got {tuple(sem_ids.shape)} "
                             f"{sem_ids.dtype}")
        return self._score_paths(batch, sem_ids, sem_ids[:, :, 0] >= 0, temperature, incremental, "score_sem_ids")

    @eval_mode
    @reset_encoder_cache
    @torch.no_grad()
    def score_items(self, batch: TokenizedSeqBatch, items: Tensor, temperature: int = 1,
                    incremental: bool = True) -> Scores:
        """log p(item | user) for C corpus items per user that the caller names: items (B, C) int64 corpus indices,
        anything outside [0, N) is padding (blocked_nodes' rule, the layout of SeqBatch.ids). The items' sem-ID rows
        come from `inference_prefix_index.cached_ids` (the trie is not needed) and are scored by score_sem_ids, which
        see: full-V softmax scores in beam_expand's arithmetic, so score_items(batch, recommend(batch, k).item_ids)
        .log_probas is recommend's log_probas (-inf in the dead places; equal to rtol 1e-5 — the kernel arithmetic is
        bitwise the same, the decoder's GEMMs round differently at another row count), and items that share a sem-ID
        row tie exactly."""
        index = getattr(self, "inference_prefix_index", None)
        if index is None or getattr(index, "cached_ids", None) is None:
            raise ValueError("score_items: requires inference_prefix_index (the tokenizer) with its corpus ids cached")
        assert self.enable_generation, "Model generation is not enabled"
        ids = index.cached_ids
        if ids.shape[1] != self.sem_id_dim:
            raise ValueError(f"score_items: the corpus rows hold {ids.shape[1]} tokens, the model generates "
                             f"{self.sem_id_dim}")
        if items.dim() != 2 or items.dtype != torch.int64:
            raise ValueError(f"score_items: items must be (B, C) int64, got {tuple(items.shape)} {items.dtype}")
        N = ids.shape[0]
        present = (items >= 0) & (items < N)
        sem_ids = torch.where(present.unsqueeze(-1), ids[items.clamp(0, max(N - 1, 0))].to(torch.int64), -1)
        return self._score_paths(batch, sem_ids, present, temperature, incremental, "score_items")

    def _score_paths(self, batch: TokenizedSeqBatch, sem_ids: Tensor, present: Tensor, temperature, incremental: bool,
                     what: str) -> Scores:
        """score_sem_ids' loop. Tokens handed back to the model are clamped into [0, V) (static shapes, no bad index
        reaches an embedding kernel); what a padding or unreachable candidate's rows compute is never read. Runs
        under the caller's decorators."""
        B, V = batch.sem_ids.shape[0], self.num_embeddings
        if sem_ids.shape[0] != B or sem_ids.shape[2] != self.sem_id_dim:
            raise ValueError(f"{what}: need {B} users and {self.sem_id_dim} tokens per candidate, got sem-ID tuples "
                             f"{tuple(sem_ids.shape)}")
        if sem_ids.device != batch.sem_ids.device:
            raise ValueError(f"{what}: the candidates must live on the batch's device {batch.sem_ids.device}, got "
                             f"{sem_ids.device}")
        C = sem_ids.shape[1]
        if not 1 <= C <= hip_ops.RANK_MAX_K:
            raise ValueError(f"{what}: need 1 <= C <= {hip_ops.RANK_MAX_K} candidates per user, got {C}")
        sem_ids, present = sem_ids.contiguous(), present.contiguous()
        lp = rank = None
        with self._step_logits(batch, incremental) as step:
            own = torch.arange(C, device=sem_ids.device).expand(B, C)
            for i in range(self.sem_id_dim):
                if i == 0:
                    logits = step()
                else:   # the BOS rows are every candidate's parent at i == 1; afterwards every candidate is its own
                    logits = step(sem_ids[:, :, :i].clamp(0, V - 1), torch.zeros_like(own) if i == 1 else own)
                lp, rank = hip_ops.score_paths(logits.contiguous(), sem_ids[:, :, i], present=present, prev_lp=lp,
                                               temperature=temperature, want_rank=i + 1 == self.sem_id_dim)
        return Scores(log_probas=lp, rank=rank)

    def _generate_constrained(self, batch: TokenizedSeqBatch, temperature, k: int, incremental: bool,
                              search: _TrieSearch):
        """_generate_sampled's loop with beam_candidates + _beam_verify + beam_select replaced by one
        `search.expand` launch per step: a beam carries its trie node, the node's children are the
        only candidates. Returns (sem_ids (B, k, L+1), log_probas (B, k), the beams' leaf nodes (B, k) int32, the
        biased scores (B, k) or None), dead beams as beam_expand marks them. Tokens handed back to the model for dead
        beams are clamped to 0 (row counts stay B * k: static shapes, no negative index reaches an embedding kernel);
        whatever they compute is never read, a dead beam has no children. `search` (_trie_search, built by the public
        call under its own name): step i skips the user's blocked level-(i + 1) nodes and, under an ItemFilter, keeps
        only the children set in its bits[i], row group[b]; under an ItemBias the steps are hip_ops.beam_expand_biased's,
        ranked by log-probability + its upper[i], row group[b] — the UNBIASED log-probability is what is carried to the
        next step as parent_lp (no bound is ever accumulated) and the last step's ranking score is kept. Runs under the
        caller's decorators."""
        B = batch.sem_ids.shape[0]
        expand = search.expand
        generated, log_probas, score, parent, node = None, None, (), None, None
        with self._step_logits(batch, incremental) as step:
            for i in range(self.sem_id_dim):
                logits = step() if generated is None else step(generated.clamp_min(0), parent)
                generated, log_probas, *score, parent, node = expand(
                    logits.contiguous(), k, batch=B, node=node, parents=generated, parent_lp=log_probas,
                    temperature=temperature, wide=None, **search.level(i))
        return generated, log_probas, node, (score[0] if score else None)

    def _beams_batch(self, cur: TokenizedSeqBatch, generated: Tensor, first: bool, k: int) -> TokenizedSeqBatch:
        """The next full forward's batch for the beams `generated` (B, k, i + 1) of _ForwardSteps: after the first
        step the users (and the cached encoder output) are repeated per beam."""
        if not first:
            nxt = generated.flatten(end_dim=1)
            return TokenizedSeqBatch(user_ids=cur.user_ids, sem_ids=cur.sem_ids, sem_ids_fut=nxt,
                                     token_type_ids_fut=torch.arange(nxt.shape[1], device=nxt.device).repeat(nxt.shape[0], 1),
                                     seq_mask=cur.seq_mask, token_type_ids=cur.token_type_ids)
        nxt = generated.reshape(-1, 1)
        enc = self.transformer.cached_enc_output
        n_ctx = cur.sem_ids.shape[1] + 1
        padded = jagged_to_padded_tensor(enc, n_ctx).repeat_interleave(k, dim=0)
        lengths = enc.offsets().diff().repeat_interleave(k)
        self.transformer.cached_enc_output = padded_to_jagged(padded.contiguous(), lengths, n_ctx)
        return TokenizedSeqBatch(user_ids=cur.user_ids.repeat_interleave(k, dim=0),
                                 sem_ids=cur.sem_ids.repeat_interleave(k, dim=0), sem_ids_fut=nxt,
                                 token_type_ids_fut=torch.zeros_like(nxt),
                                 seq_mask=cur.seq_mask.repeat_interleave(k, dim=0),
                                 token_type_ids=cur.token_type_ids.repeat_interleave(k, dim=0))

    def _beam_verify(self, index, i: int, cand_ids: Tensor, generated, n_cand: int) -> dict:
        """hip_ops.beam_select's validity arguments for step i's candidates: the tokenizer's packed-prefix table
        when `inference_prefix_index` is set, else `inference_verifier_fn` on the materialised prefixes."""
        if index is not None:
            from modules.tokenizer.semids import BATCH_SIZE
            keys, base = index.prefix_table(i + 1)
            # exists_prefix's batching quirk acts on the prefix tensor's leading axis: here the B * kprev logits
            # rows (n_cand candidates each), of which the last partial batch of 16 goes unchecked
            rows = cand_ids.shape[0]
            return dict(keys=keys, base=base,
                        checked=(rows // BATCH_SIZE * BATCH_SIZE if index.reference_batching else rows) * n_cand)
        if generated is None:
            valid = self.inference_verifier_fn(cand_ids.unsqueeze(-1))
        else:
            prefix = torch.cat([generated.flatten(0, 1).unsqueeze(1).repeat_interleave(n_cand, axis=1),
                                cand_ids.unsqueeze(-1)], axis=-1)
            valid = self.inference_verifier_fn(prefix)
        return dict(valid=valid.to(torch.bool).reshape(-1).contiguous())

    @contextlib.contextmanager
    def _step_logits(self, batch: TokenizedSeqBatch, incremental: bool):
        """The per-step logits of every decoding loop below, as a callable: step() gives the B BOS rows' logits,
        step(beams, parent) those of the beams (B, k, i) int64 kept so far (tokens the model can embed: clamping is the
        caller's), parent (B, k) each beam's index among the previous step's. incremental: one BeamDecodeState under
        one weight split for the whole call; else full forwards (forward opens a weight split per call)."""
        if incremental:
            with hip_ops.weight_split_scope(self._gemm_weights(), self._gemm_weight_stacks()):
                yield _IncrementalSteps(BeamDecodeState(self, batch))
        else:
            yield _ForwardSteps(self, batch)

    def _generate_sampled(self, batch: TokenizedSeqBatch, temperature, top_k: bool, sample: bool,
                          incremental: bool) -> GenerationOutput:
        """generate_next_sem_id with the per-step beam logic on hip_ops.beam_candidates (softmax, the draw, the
        candidates' log-probabilities) and hip_ops.beam_select (verification, cumulative score, stable top-k,
        parent gather). The draw: the n_cand largest p / e with e ~ Exponential(1) from torch's generator — the
        distribution of torch.multinomial without replacement; sample=False: the n_cand largest p. Prefixes are
        verified in the select kernel against `inference_prefix_index.prefix_table` (the tokenizer's sorted
        packed-prefix keys, incl. its reference_batching quirk) when that attribute is set, else by
        `inference_verifier_fn` on the materialised prefixes. incremental: the logits come from BeamDecodeState
        steps (_step_logits) — the same calls, verification and noise draws on logits of the same shapes — and the
        select launch also returns each winner's parent beam, which is all the state needs to follow the beams (the
        full-forward form does not ask for it: no output it never reads). Runs under generate_next_sem_id's
        decorators."""
        B = batch.sem_ids.shape[0]
        k = 32 if top_k else 1
        n_cand = 200 if top_k else 1
        index = getattr(self, "inference_prefix_index", None)
        generated, log_probas, parent = None, None, ()
        with self._step_logits(batch, incremental) as step:
            for i in range(self.sem_id_dim):
                logits = (step() if generated is None else step(generated, *parent)).contiguous()
                noise = torch.empty_like(logits).exponential_() if sample else None
                cand_ids, cand_lp = hip_ops.beam_candidates(logits, n_cand, temperature, noise)
                verify = self._beam_verify(index, i, cand_ids, generated, n_cand)
                generated, log_probas, *parent = hip_ops.beam_select(cand_ids, cand_lp, k, batch=B, parents=generated,
                                                                     parent_lp=log_probas, return_parent=incremental,
                                                                     **verify)
        return GenerationOutput(sem_ids=generated.squeeze(), log_probas=log_probas.squeeze())


class _ForwardSteps:
    """_step_logits by full forwards: owns the batch, which grows by the beams' tokens. The next batch
    (_beams_batch) is built when the next step is asked for, so nothing is built after the last token."""

    def __init__(self, model: EncoderDecoderRetrievalModel, batch: TokenizedSeqBatch) -> None:
        self.model = model
        self.cur = TokenizedSeqBatch(user_ids=batch.user_ids, sem_ids=batch.sem_ids, sem_ids_fut=None,
                                     seq_mask=batch.seq_mask, token_type_ids=batch.token_type_ids,
                                     token_type_ids_fut=None)

    def __call__(self, beams: Tensor = None, parent: Tensor = None) -> Tensor:
        if beams is not None:   # parent is not needed: a beam's row holds its whole prefix
            self.cur = self.model._beams_batch(self.cur, beams, self.cur.sem_ids_fut is None, beams.shape[1])
        return self.model.forward(self.cur).logits


class _IncrementalSteps:
    """_step_logits by a BeamDecodeState: passes on the beams' newest token column and their parent indices."""

    def __init__(self, state: "BeamDecodeState") -> None:
        self.state = state

    def __call__(self, beams: Tensor = None, parent: Tensor = None) -> Tensor:
        return self.state.step() if beams is None else self.state.step(beams[:, :, -1], parent)


class BeamDecodeState:
    """Incremental beam decoding of an eval-mode EncoderDecoderRetrievalModel for one batch of B users.

    Construction runs the encoder once and projects every decoder layer's cross-attention K / V once, from the B
    un-repeated contexts (cross-attention is not causal and a user's beams attend the same keys). `step()` pushes
    the B BOS rows through the decoder and returns logits (B, K); `step(tokens, parent)` then takes each kept
    beam's newest token (B, k) int64 and its parent beam index (B, k) in [0, kprev) — hip_ops.beam_select(
    return_parent=True) — and returns logits (B * k, K), b-major. Only the newest token of every beam runs through
    the decoder: self-attention is causal and the block's other ops are row-wise, so earlier tokens enter only
    through their self-attention K / V. Those stay in each step's packed qkv output where they were written; an
    ancestor row table (hip_ops.beam_advance_ancestors) follows the beams through every re-ordering, so no cache
    is gathered or appended. The state holds its tensors for one generation call; drop it afterwards."""

    @torch.no_grad()
    def __init__(self, model: EncoderDecoderRetrievalModel, batch: TokenizedSeqBatch) -> None:
        assert not model.training, "BeamDecodeState: eval mode only"
        assert model.sem_id_dim <= hip_ops.BEAM_MAX_T, "BeamDecodeState: sem_id_dim exceeds RQ_BEAM_MAX_T"
        self.model = model
        self.B = batch.sem_ids.shape[0]
        tr = model.transformer
        enc = tr.encoder(model._context_inputs(batch), padding_mask=batch.seq_mask, is_causal=False, context=None,
                         jagged=True)
        self.cross_kvs = tr.decoder.cross_kv(enc)
        self.cu_k, self.max_k = enc.offsets(), enc.max_len
        self.self_kv = [[] for _ in tr.decoder.layers]   # per layer: one (k, v) view pair per step so far
        self.anc = None      # (rows, t) int32: each current beam's row in every earlier step
        self.rows = self.B   # rows of the previous step
        self.t = 0           # tokens pushed so far (BOS included)

    @torch.no_grad()
    def step(self, tokens: Tensor = None, parent: Tensor = None) -> Tensor:
        m, B = self.model, self.B
        assert self.t < m.sem_id_dim, "BeamDecodeState: every token of the sem-ID has been decoded"
        if self.t == 0:
            assert tokens is None and parent is None, "BeamDecodeState: the first step takes no tokens"
            group = 1
            x = m.bos_emb.unsqueeze(0).expand(B, -1).contiguous()
        else:
            assert tokens.shape == parent.shape and tokens.shape[0] == B
            group, j = tokens.shape[1], self.t - 1
            # the j-th generated token: sem-ID table row j K + token plus token-type row j (token_type_ids_fut)
            x = m.sem_id_embedder.emb((j * m.num_embeddings + tokens).reshape(-1)) + m.tte.weight[j]
            self.anc = hip_ops.beam_advance_ancestors(self.anc, parent, self.rows // B)
        x = m.in_proj(m.norm_cxt(x))
        cu_q = torch.arange(B + 1, device=x.device, dtype=self.cu_k.dtype) * group
        h = m.transformer.decoder.decode_step(x, self.self_kv, self.anc, self.cross_kvs, cu_q, self.cu_k, group,
                                              self.max_k)
        self.t += 1
        self.rows = B * group
        return m.out_proj(h)
