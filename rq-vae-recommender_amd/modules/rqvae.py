"""RQ-VAE — drop-in for reference modules/rqvae.py (RqVaeOutput :22-26, RqVaeComputedLosses
:29-34, RqVae :37-165; same constructor, methods, outputs and state-dict keys
``encoder.mlp.*``, ``decoder.mlp.*``, ``layers.{l}.embedding.weight``).

Hot path: ``get_semantic_ids`` runs all L levels in ONE fused HIP launch
(rqvae_hip.ops.rq_quantize: MFMA fp32 cdist -> argmin -> rotation trick / STE / eval -> VQ loss
-> residual update, chained on-chip) and its VJP with a deterministic codebook gradient.
``p_unique_ids`` uses a hash-count kernel (O(B L)) instead of the reference's O(B^2 L) mask.
The reference wraps forward in torch.compile(mode="reduce-overhead"); this build instead
exposes a whole-step hipGraph capture (rqvae_hip.graph) and never invokes inductor.
"""
from typing import List, NamedTuple

import torch
from torch import nn
from torch import Tensor

from data.schemas import SeqBatch
from modules.encoder import MLP
from modules.loss import CategoricalReconstuctionLoss, ReconstructionLoss
from modules.normalize import L2NormalizationLayer, l2norm
from modules.quantize import Quantize, QuantizeDistance, QuantizeForwardMode, fused_mode
from rqvae_hip import ops as hip_ops

# As the reference (modules/rqvae.py:19): fp32 matmuls at 'high' precision. On gfx950 (no xf32)
# the MLP matmuls then run split-bf16 (rqvae_hip.ops.gemm_bf16x3); 'highest' restores exact fp32.
torch.set_float32_matmul_precision('high')


class RqVaeOutput(NamedTuple):
    embeddings: Tensor      # (B, D, L)
    residuals: Tensor       # (B, D, L)
    sem_ids: Tensor         # (B, L) int64
    quantize_loss: Tensor   # (B,)


class RqVaeBeamOutput(NamedTuple):
    sem_ids: Tensor         # (B, W, L) int64, beams ascending by error
    errors: Tensor          # (B, W)
    residuals: Tensor       # (B, W, D)


class RqVaeComputedLosses(NamedTuple):
    loss: Tensor
    reconstruction_loss: Tensor
    rqvae_loss: Tensor
    embs_norm: Tensor       # (B, L)
    p_unique_ids: Tensor    # 0-d float


class RqVae(nn.Module):
    def __init__(
        self,
        input_dim: int,
        embed_dim: int,
        hidden_dims: List[int],
        codebook_size: int,
        codebook_kmeans_init: bool = True,
        codebook_normalize: bool = False,
        codebook_sim_vq: bool = False,
        codebook_mode: QuantizeForwardMode = QuantizeForwardMode.GUMBEL_SOFTMAX,
        n_layers: int = 3,
        commitment_weight: float = 0.25,
        n_cat_features: int = 18,
    ) -> None:
        # plain kwargs (the reference pickles `self` via locals(); SURVEY A-13)
        self._config = dict(input_dim=input_dim, embed_dim=embed_dim, hidden_dims=list(hidden_dims),
                            codebook_size=codebook_size, codebook_kmeans_init=codebook_kmeans_init,
                            codebook_normalize=codebook_normalize, codebook_sim_vq=codebook_sim_vq,
                            codebook_mode=codebook_mode, n_layers=n_layers, commitment_weight=commitment_weight,
                            n_cat_features=n_cat_features)
        super().__init__()
        self.input_dim = input_dim
        self.embed_dim = embed_dim
        self.hidden_dims = hidden_dims
        self.n_layers = n_layers
        self.codebook_size = codebook_size
        self.commitment_weight = commitment_weight
        self.n_cat_feats = n_cat_features
        self.layers = nn.ModuleList([
            Quantize(embed_dim=embed_dim, n_embed=codebook_size, forward_mode=codebook_mode,
                     do_kmeans_init=codebook_kmeans_init, codebook_normalize=(i == 0 and codebook_normalize),
                     sim_vq=codebook_sim_vq, commitment_weight=commitment_weight)
            for i in range(n_layers)
        ])
        self.encoder = MLP(input_dim=input_dim, hidden_dims=hidden_dims, out_dim=embed_dim,
                           normalize=codebook_normalize)
        self.decoder = MLP(input_dim=embed_dim, hidden_dims=list(hidden_dims)[::-1], out_dim=input_dim,
                           normalize=True)
        self.reconstruction_loss = (CategoricalReconstuctionLoss(n_cat_features) if n_cat_features != 0
                                    else ReconstructionLoss())
        self.code_usage = None   # (L, K) int64 usage counters while track_usage() is on; never a buffer
        self.ema = None          # use_ema_codebooks(): dict(decay, eps, N, S, n, s); plain tensors, never buffers

    @property
    def config(self) -> dict:
        return self._config

    @property
    def device(self) -> torch.device:
        return next(self.encoder.parameters()).device

    def load_pretrained(self, path: str) -> None:
        """Load a checkpoint {"iter", "model", ...}. Only tensor payloads are accepted
        (weights_only=True): reference checkpoints that pickle the module object itself must be
        re-saved as a plain state dict first."""
        state = torch.load(path, map_location=self.device, weights_only=True)
        self.load_state_dict(state["model"])
        print(f"---Loaded RQVAE Iter {state['iter']}---")

    def encode(self, x: Tensor) -> Tensor:
        return self.encoder(x)

    def decode(self, x: Tensor) -> Tensor:
        return self.decoder(x)

    # ----------------------------------------------------------------- semantic ids
    def _fused_kernel_mode(self):
        modes = {fused_mode(layer.forward_mode, self.training) for layer in self.layers}
        if len(modes) != 1 or None in modes:
            return None
        if any(layer.distance_mode != QuantizeDistance.L2 or layer.needs_init() for layer in self.layers):
            return None
        return modes.pop()

    def quantize_levels(self, res0: Tensor, gumbel_t: float, with_norms: bool = False):
        """All levels -> (emb (L,B,D), res (L,B,D), ids (B,L), qloss (B,), emb_sum (B,D)
        [, |emb| (L,B) without grad when with_norms])."""
        mode = self._fused_kernel_mode()
        if mode is not None:
            if all(isinstance(m, nn.Identity) for layer in self.layers for m in layer.out_proj):   # codebook() == weight
                codebooks = hip_ops.stack_params([layer.embedding.weight for layer in self.layers])
            else:
                codebooks = torch.stack([layer.codebook() for layer in self.layers])
            return hip_ops.rq_quantize(res0, codebooks, mode, self.commitment_weight, with_norms)
        # generic per-level path (k-means init pending, gumbel / cosine layers)
        res, qloss = res0, 0
        embs, ress, ids = [], [], []
        for layer in self.layers:
            ress.append(res)
            q = layer(res, temperature=gumbel_t)
            qloss = qloss + q.loss
            res = res - q.embeddings
            embs.append(q.embeddings)
            ids.append(q.ids)
        emb = torch.stack(embs)
        out = (emb, torch.stack(ress), torch.stack(ids, 1), qloss, emb.sum(0))
        if with_norms:
            with torch.no_grad():
                out += (hip_ops.row_norms(emb),)     # emb.norm(dim=-1) over (L, B, D)
        return out

    def get_semantic_ids(self, x: Tensor, gumbel_t: float = 0.001) -> RqVaeOutput:
        emb, res, ids, qloss, _ = self.quantize_levels(self.encode(x), gumbel_t)
        return RqVaeOutput(embeddings=emb.permute(1, 2, 0), residuals=res.permute(1, 2, 0), sem_ids=ids,
                           quantize_loss=qloss)

    @torch.no_grad()
    def get_semantic_id_beams(self, x: Tensor, width: int) -> RqVaeBeamOutput:
        """The `width` best code paths of every item instead of the greedy one (an extension: beam-searched residual
        quantization, modules.beam_quantize) -> RqVaeBeamOutput, beams sorted by reconstruction error in the code
        space; width = 1 is get_semantic_ids' rule. Device tensors run one HIP launch (rqvae_hip.ops.rq_quantize_beam),
        CPU tensors the torch restatement. Codebooks are used as in eval mode: L2-distance levels whose k-means init
        is done, and not a training-mode model whose forward mode differs from its eval forward. No gradient."""
        for layer in self.layers:
            if layer.distance_mode != QuantizeDistance.L2:
                raise ValueError("get_semantic_id_beams: needs L2-distance levels")
            if layer.needs_init():
                raise ValueError("get_semantic_id_beams: the k-means init of the codebooks is still pending")
        if any(fused_mode(layer.forward_mode, self.training) != hip_ops.MODE_EVAL for layer in self.layers):
            raise ValueError("get_semantic_id_beams: the model is in training mode with a non-eval forward mode; "
                             "call eval() first")
        codebooks = torch.stack([layer.codebook() for layer in self.layers])
        res0 = self.encode(x)
        if res0.is_cuda:
            paths, err, res = hip_ops.rq_quantize_beam(res0, codebooks, width, with_residuals=True)
        else:
            from modules.beam_quantize import beam_quantize_torch
            paths, err, res = beam_quantize_torch(res0, codebooks, width)
        return RqVaeBeamOutput(sem_ids=paths, errors=err, residuals=res)

    def forward(self, batch: SeqBatch, gumbel_t: float) -> RqVaeComputedLosses:
        # every encoder / decoder GEMM weight split once for the step, in one launch (the fused chains take
        # their planes from the scope; two chains split separately were two launches)
        weights = [m.weight for mlp in (self.encoder.mlp, self.decoder.mlp) for m in mlp if isinstance(m, nn.Linear)]
        with hip_ops.weight_split_scope(weights):
            return self._forward(batch, gumbel_t)

    def _forward(self, batch: SeqBatch, gumbel_t: float) -> RqVaeComputedLosses:
        x = batch.x
        # the level loop also returns embs_norm = |emb_l| (modules/rqvae.py:151 of the reference),
        # written from the fused kernel's level epilogue
        emb, res, ids, qloss, emb_sum, emb_norms = self.quantize_levels(self.encode(x), gumbel_t, with_norms=True)
        n = self.n_cat_feats
        head = self.decoder.mlp
        if n == 0 and isinstance(head[-1], L2NormalizationLayer) and x.dtype == torch.float32:
            fused = self.decoder._fused_chain(emb_sum)
            if fused is not None and x.shape[-1] % 4 == 0:
                # 'high': the decoder MLP chain + l2norm + ReconstructionLoss as one node whose
                # backward hands the split output gradient straight to the chain's GEMMs
                reconstruction = hip_ops.mlp_l2norm_recon(emb_sum, x, fused[0], fused[1])
            else:
                # decoder's final l2norm + ReconstructionLoss fused into one HIP row kernel (fwd + bwd)
                reconstruction = hip_ops.l2norm_recon_loss(self.decoder.body(emb_sum), x)
        else:
            x_hat = self.decode(emb_sum)
            if n > 0:   # the reference's cat is a no-op for n == 0 (SURVEY A-10)
                x_hat = torch.cat([l2norm(x_hat[..., :-n]), x_hat[..., -n:]], axis=-1)
            reconstruction = self.reconstruction_loss(x_hat, x)
        # loss = mean(recon + qloss) and the two logged means in one deterministic pass
        loss, recon_mean, rq_mean = hip_ops.loss_means(reconstruction, qloss)
        with torch.no_grad():
            embs_norm = emb_norms.T
            p_unique_ids = hip_ops.unique_fraction(ids, self.codebook_size)
            if self.code_usage is not None and self.training:
                hip_ops.code_usage(ids, self.code_usage)
            if self.ema is not None and self.training:
                from modules.codebook_ema import ema_stats_
                ema_stats_(res, ids, self.ema["n"], self.ema["s"])
        return RqVaeComputedLosses(loss=loss, reconstruction_loss=recon_mean, rqvae_loss=rq_mean,
                                   embs_norm=embs_norm, p_unique_ids=p_unique_ids)

    # ------------------------------------------------- codebook usage and dead-code revival (extensions)
    def track_usage(self, enable: bool = True) -> None:
        """Count, per level, how often each code is selected by TRAINING forwards (eval forwards do not count):
        `self.code_usage`, int64 (L, K) on the model's device, grows by one rq_code_usage launch per forward
        (captured with a graphed step). The counters are allocated here, never inside a step, and are a plain
        attribute, not a registered buffer: state_dict() keeps the reference's keys. enable=False drops them."""
        self.code_usage = (torch.zeros((self.n_layers, self.codebook_size), dtype=torch.int64, device=self.device)
                           if enable else None)

    def usage_stats(self):
        """(used, perplexity), two lists of L floats: the fraction of each level's codes with a non-zero count and
        exp(H) of the level's normalised counts (K for a uniformly used codebook, 1 for a collapsed one, 0 before
        anything was counted). Plain torch, for log time."""
        if self.code_usage is None:
            raise ValueError("usage_stats: call track_usage() first")
        c = self.code_usage.to(torch.float64)
        p = c / c.sum(1, keepdim=True).clamp_min(1.0)
        ent = -(p * torch.log(p.clamp_min(1e-300))).sum(1)
        ppl = torch.where(c.sum(1) > 0, torch.exp(ent), torch.zeros_like(ent))
        return (c > 0).to(torch.float64).mean(1).tolist(), ppl.tolist()

    def revive_dead_codes(self, x: Tensor, *, min_count: int = 1, seed: int, optimizer=None,
                          ema_min_count: float = None) -> Tensor:
        """Re-seat every codeword counted fewer than min_count times since the counters were last zeroed on the
        residual of a row of x (modules.codebook_revival.revive_: the rule, the data-parallel protocol) ->
        n_revived (L,) int64; zeroes the counters. x (B >= K, input_dim): data rows; their level inputs come from
        one eval-mode, no-grad quantize_levels(encode(x)) under the PRE-revival codebooks — the residuals of deeper
        levels are knowingly not recomputed after a shallower level is re-seated, so a deeper donor is a residual
        the old shallower codebook left. optimizer: when given, the exp_avg / exp_avg_sq rows of the re-seated
        codewords are zeroed too (if that state exists yet). Parameters and moments are written through their
        existing storage, so captured graphs stay valid. L2-distance levels without out_proj only.
        ema_min_count (EMA codebooks only): the dead set is {k : N[l][k] < ema_min_count}, the decayed usage of the
        EMA state, instead of the window counters (track_usage() is then not needed; N is identical on every rank).
        After any revival with EMA codebooks on, the re-seated rows restart at N = 1, S = W."""
        from modules.codebook_revival import revive_
        if ema_min_count is not None and self.ema is None:
            raise ValueError("revive_dead_codes: ema_min_count needs use_ema_codebooks()")
        if ema_min_count is None and self.code_usage is None:
            raise ValueError("revive_dead_codes: call track_usage() first")
        for layer in self.layers:
            if not all(isinstance(m, nn.Identity) for m in layer.out_proj):
                raise ValueError("revive_dead_codes: codebooks with an out_proj (sim_vq / codebook_normalize) are not "
                                 "supported")
            if layer.distance_mode != QuantizeDistance.L2 or layer.needs_init():
                raise ValueError("revive_dead_codes: needs L2-distance levels whose k-means init is done")
        if x.dim() != 2 or x.shape[0] < self.codebook_size:
            raise ValueError(f"revive_dead_codes: x must hold at least K = {self.codebook_size} rows, got "
                             f"{tuple(x.shape)}")
        was_training = self.training
        self.eval()
        try:
            with torch.no_grad():
                res = self.quantize_levels(self.encode(x), 0.001)[1].contiguous()
        finally:
            self.train(was_training)
        weights = [layer.embedding.weight for layer in self.layers]
        moments = None
        if optimizer is not None:
            states = [optimizer.state.get(w, {}) for w in weights]
            if all("exp_avg" in st and "exp_avg_sq" in st for st in states):
                moments = ([st["exp_avg"] for st in states], [st["exp_avg_sq"] for st in states])
        import torch.distributed as dist
        dead = None
        if ema_min_count is None:
            counts = self.code_usage
            if self.ema is not None:   # the dead set revive_ will see: the counters summed over the ranks
                total = counts.clone()
                if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
                    dist.all_reduce(total, op=dist.ReduceOp.SUM)
                dead = total < min_count
        else:
            # dead <=> N < ema_min_count, as counters for revive_'s `counts < min_count`; N is the same on every
            # rank, so the ranks' sum (world x these) keeps the dead set: dead codes stay 0
            counts, min_count = (self.ema["N"] >= float(ema_min_count)).to(torch.int64), 1
            dead = counts < min_count
        n_rev = revive_(weights, counts, res, min_count=min_count, seed=seed,
                        exp_avg=moments and moments[0], exp_avg_sq=moments and moments[1])
        if self.ema is not None:
            N, S = self.ema["N"], self.ema["S"]
            for l, w in enumerate(weights):
                # copies and a constant: the ranks still agree bit for bit
                N[l] = torch.where(dead[l], torch.ones_like(N[l]), N[l])
                S[l] = torch.where(dead[l][:, None], w.detach(), S[l])
        return n_rev

    # ---------------------------------------------------------------- EMA-maintained codebooks (extension)
    def use_ema_codebooks(self, decay: float = 0.99, eps: float = 1e-5) -> None:
        """Maintain the codebooks as an exponential moving average of the residuals assigned to them
        (modules.codebook_ema: the rule, the data-parallel protocol) instead of by the optimizer: every TRAINING
        forward adds its per-code counts and residual sums into `self.ema["n"]`, `self.ema["s"]` (one
        codebook_ema_stats call, captured with a graphed step; eval forwards do not), and `ema_update()` — once per
        optimizer step, eagerly, after `opt.step()` — applies the update. The L codebook weights stop requiring a
        gradient, so gradient buckets and AdamW (and its weight decay) leave them alone: call this BEFORE the
        buckets and the optimizer are built and before the first captured step. With torch.distributed initialised
        and more than one rank the codebooks are broadcast from rank 0 here (the buckets no longer do). The state
        N (L, K), S (L, K, D) starts as N = 1, S = W; like `code_usage` it is a plain attribute, not a buffer:
        state_dict() keeps the reference's keys (ema_state_dict() / load_ema_state_dict() for checkpoints). The loss
        values and the encoder's commitment gradient are unchanged. L2-distance levels without out_proj whose
        k-means init is done, forward mode STE or ROTATION_TRICK."""
        import torch.distributed as dist
        from modules.codebook_ema import initial_state
        hip_ops.ema_check_args(self.n_layers, self.codebook_size, self.embed_dim, float(decay), float(eps),
                               "use_ema_codebooks")
        for layer in self.layers:
            if not all(isinstance(m, nn.Identity) for m in layer.out_proj):
                raise ValueError("use_ema_codebooks: codebooks with an out_proj (sim_vq / codebook_normalize) are not "
                                 "supported")
            if layer.distance_mode != QuantizeDistance.L2:
                raise ValueError("use_ema_codebooks: needs L2-distance levels")
            if layer.needs_init():
                raise ValueError("use_ema_codebooks: the k-means init of the codebooks is still pending")
            if layer.forward_mode not in (QuantizeForwardMode.STE, QuantizeForwardMode.ROTATION_TRICK):
                raise ValueError("use_ema_codebooks: the forward mode must be STE or ROTATION_TRICK, got "
                                 f"{layer.forward_mode}")
        weights = [layer.embedding.weight for layer in self.layers]
        for w in weights:
            w.requires_grad_(False)
            w.grad = None
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            for w in weights:
                dist.broadcast(w.data, src=0)
        N, S, n, s = initial_state(weights)
        self.ema = dict(decay=float(decay), eps=float(eps), N=N, S=S, n=n, s=s)

    def _ema(self, what: str) -> dict:
        if self.ema is None:
            raise ValueError(f"{what}: call use_ema_codebooks() first")
        return self.ema

    def ema_update(self, group=None) -> None:
        """One EMA update of the codebooks from the statistics accumulated since the last one (summed over the
        data-parallel ranks first); zeroes the statistics. Writes the weights through their existing storage, so
        captured graphs stay valid."""
        from modules.codebook_ema import ema_apply_
        e = self._ema("ema_update")
        ema_apply_([layer.embedding.weight for layer in self.layers], e["N"], e["S"], e["n"], e["s"],
                   decay=e["decay"], eps=e["eps"], group=group)

    def ema_discard_stats(self) -> None:
        """Zero the accumulated statistics without an update (e.g. after the warm-up passes of a step capture,
        which run training forwards on the step's batch)."""
        e = self._ema("ema_discard_stats")
        e["n"].zero_()
        e["s"].zero_()

    def ema_state_dict(self) -> dict:
        """{"decay", "eps", "N", "S"}: what a checkpoint needs beside state_dict() (the statistics of an unfinished
        step are not part of it)."""
        e = self._ema("ema_state_dict")
        return {"decay": e["decay"], "eps": e["eps"], "N": e["N"].clone(), "S": e["S"].clone()}

    def load_ema_state_dict(self, state: dict) -> None:
        """Restore ema_state_dict()'s result (after use_ema_codebooks(); decay and eps are taken from `state`)."""
        e = self._ema("load_ema_state_dict")
        if tuple(state["N"].shape) != tuple(e["N"].shape) or tuple(state["S"].shape) != tuple(e["S"].shape):
            raise ValueError(f"load_ema_state_dict: N / S must be {tuple(e['N'].shape)} / {tuple(e['S'].shape)}, got "
                             f"{tuple(state['N'].shape)} / {tuple(state['S'].shape)}")
        hip_ops.ema_check_args(self.n_layers, self.codebook_size, self.embed_dim, float(state["decay"]),
                               float(state["eps"]), "load_ema_state_dict")
        e["decay"], e["eps"] = float(state["decay"]), float(state["eps"])
        e["N"].copy_(state["N"])
        e["S"].copy_(state["S"])
        e["n"].zero_()
        e["s"].zero_()
