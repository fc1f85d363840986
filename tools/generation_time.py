#!/usr/bin/env python3
"""Time of one eval batch of the decoder trainer at the Amazon shape (B = 256 sequences, 32 beams, 200 candidates
per beam, 256 classes, 4 sem-ID tokens; model dims of configs/decoder_amazon.gin):

  generation   generate_next_sem_id(top_k=True) with fused=False (the reference's torch composition of the beam
               step), fused=True (rq_beam_candidates + rq_beam_select) and fused=True, incremental=True (the same
               beam step over a BeamDecodeState: cross K/V projected once per user, only each beam's newest token
               through the decoder), and fused=True, incremental=True, constrained=True, sample=False (the
               incremental loop with the beam step replaced by one rq_beam_expand launch that walks the corpus'
               prefix trie) and the same call with exclude_items (`excluded`: H = the batch's history length of 20
               items per user, drawn from the corpus, padded where the sequence is; one rq_trie_blocked_nodes launch
               per call and rq_beam_expand with its blocked rows per step), verifier = a tokenizer over a 12,101-item
               corpus; and with the beam step
               stubbed out (`model`: the four forwards and the encoder cache repeat alone), which gives the
               beam logic's share of the first two forms;
  scoring      `recommend`: model.recommend(k=10) (the constrained incremental search); `score`: model.score_items
               with --score-candidates (100) corpus items per user drawn from the corpus (one BeamDecodeState, one
               rq_score_paths launch per step); `score_full`: the same with incremental=False (full forwards over
               B C rows) at --score-full-candidates per user (default: the same C; the JSON states both);
               `wide`: model.recommend(k=min(100, beams), beams=--beams (128)) — past 32 beams at V = 256 the steps
               after the first run rq_beam_expand_wide; `wide_excluded`: the same call with `excluded`'s histories;
               `recommend_forced`: `recommend` with every beam_expand call handed to the wide kernel (wide=True), so
               one trace of the two forms times both kernels at the 32-beam shape;
               `sampled_items`: model.sample_items(k=10) — stochastic beam search, the incremental loop 10 beams wide
               with one Exponential(1) draw and one rq_beam_expand_sampled launch per step;
  filters      `filtered_shared`: model.recommend(k=10, item_filter=F) with F one ItemFilter over a 50 % mask of the
               corpus that every user shares, built once before the loop (rq_beam_expand with allowed / group per step);
               `filtered_groups`: the same call with one 50 % mask per user (G = B groups, filter_group = 0..B-1);
               `filter_build`: the one-off tokenizer.item_filter(mask) of the shared mask, `filter_build_groups` of
               the G = B masks (rq_trie_allowed_nodes: two launches). The over-fetch alternative is `wide`. One run
               for the comparison:
                 --forms recommend,filtered_shared,filtered_groups,wide,filter_build,filter_build_groups
               (the JSON then carries `filtered_vs_recommend`: each filtered form's median over `recommend`'s, next
               to `recommend`'s own min..max spread);
  accumulate   TopKAccumulator.accumulate on the device (one rq_topk_hits launch) and the reference's logic
               (evaluate/metrics.py:15-28, restated below: 24 host reads per batch).

Each form is warmed up, then timed `--reps` times with the forms alternating; a span is a host clock around work
that ends in a device synchronise. Prints one JSON line (medians, ms; `peak_mem_mib`: torch.cuda.max_memory_allocated
over one further call of each generation form). `--forms A,B` alternates only those forms. `--only FORM --reps N --warmup 0` runs a single form N times for a
kernel trace (rocprofv3 --kernel-trace --stats -- python tools/generation_time.py ...), after the set-up's one
fused call: launches per beam step = (calls of the form - calls of `model`) / (4 N).
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "rq-vae-recommender_amd")]

import torch  # noqa: E402


def reference_accumulate(metrics, ks, actual, top_k):
    """The reference accumulator's arithmetic on whatever device the tensors live on (a len() per counter)."""
    B, D = actual.shape
    pos_match = actual.unsqueeze(1) == top_k
    for i in range(D):
        match_found, rank = pos_match[..., :i + 1].all(axis=-1).max(axis=-1)
        matched_rank = rank[match_found]
        for k in ks:
            metrics[f"h@{k}_slice_:{i + 1}"] = metrics.get(f"h@{k}_slice_:{i + 1}", 0) + len(matched_rank[matched_rank < k])
        match_found, rank = pos_match[..., i:i + 1].all(axis=-1).max(axis=-1)
        matched_rank = rank[match_found]
        for k in ks:
            metrics[f"h@{k}_pos_{i}"] = metrics.get(f"h@{k}_pos_{i}", 0) + len(matched_rank[matched_rank < k])


def build(device, B, seed=0):
    from data.processed import synthetic_tokenized_batch
    from modules.model import EncoderDecoderRetrievalModel
    from modules.tokenizer.semids import SemanticIdTokenizer, dedup_rank
    K, L1, n_items = 256, 4, 12101
    tok = SemanticIdTokenizer(input_dim=8, output_dim=4, hidden_dims=[8], codebook_size=K, n_layers=L1 - 1, n_cat_feats=0)
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(0, K, (n_items, L1 - 1), generator=g).to(device)
    tok.cached_ids = torch.cat([ids, dedup_rank(ids).unsqueeze(1)], 1)
    torch.manual_seed(seed)
    model = EncoderDecoderRetrievalModel(embedding_dim=128, attn_dim=512, dropout=0.3, num_heads=8, n_layers=8,
                                         num_embeddings=K, sem_id_dim=L1,
                                         inference_verifier_fn=lambda x: tok.exists_prefix(x), max_pos=20 * L1).to(device)
    model.enable_generation = True
    model.inference_prefix_index = tok
    model.eval()
    return model, tok, synthetic_tokenized_batch(B, 20, L1, K, seed + 1, device)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    names = ["unfused", "fused", "incremental", "constrained", "excluded", "model", "acc_device", "acc_reference",
             "recommend", "score", "score_full", "wide", "wide_excluded", "recommend_forced", "sampled_items",
             "filtered_shared", "filtered_groups", "filter_build", "filter_build_groups", "biased", "bias_build",
             "bias_build_groups"]
    ap.add_argument("--score-candidates", type=int, default=100)
    ap.add_argument("--score-full-candidates", type=int, default=None)
    ap.add_argument("--beams", type=int, default=128, help="width of the `wide` / `wide_excluded` search")
    ap.add_argument("--only", choices=names)
    ap.add_argument("--forms", type=lambda v: v.split(","), help="comma-separated subset of the forms to alternate")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("generation_time: needs the GPU (a CPU run measures nothing)")
    from evaluate.metrics import TopKAccumulator
    from rqvae_hip import ops as hip_ops
    device = torch.device("cuda", 0)
    model, tok, batch = build(device, args.batch)
    B, k, n_cand, L1 = args.batch, 32, 200, 4
    real = (hip_ops.beam_candidates, hip_ops.beam_select)
    expand = hip_ops.beam_expand

    def recommend_forced():
        hip_ops.beam_expand = lambda *a, **kw: expand(*a, **{**kw, "wide": True})
        try:
            return model.recommend(batch, k=10)
        finally:
            hip_ops.beam_expand = expand

    fixed = {}   # the stubbed beam step's outputs, allocated once

    def stub_candidates(logits, n, temperature=1.0, noise=None):
        key = ("c", logits.shape[0])
        if key not in fixed:
            fixed[key] = (torch.zeros((logits.shape[0], n), dtype=torch.int64, device=device),
                          torch.zeros((logits.shape[0], n), device=device))
        return fixed[key]

    def stub_select(cand_ids, cand_lp, kk, *, batch, parents=None, **_):
        P = 0 if parents is None else parents.shape[2]
        if P not in fixed:
            fixed[P] = (torch.zeros((batch, kk, P + 1), dtype=torch.int64, device=device),
                        torch.zeros((batch, kk), device=device))
        return fixed[P]

    def gen(fused, incremental=False):
        return model.generate_next_sem_id(batch, temperature=1, top_k=True, fused=fused, incremental=incremental)

    def gen_constrained():
        return model.generate_next_sem_id(batch, temperature=1, top_k=True, fused=True, sample=False, incremental=True,
                                          constrained=True)

    # one history per user: as many corpus items as the sequence holds (its mask), -1 behind them
    L1_ = model.sem_id_dim
    n_hist = batch.seq_mask.shape[1] // L1_
    seen = torch.randint(0, tok.cached_ids.shape[0], (args.batch, n_hist),
                         generator=torch.Generator().manual_seed(7)).to(device)
    seen = seen.masked_fill(~batch.seq_mask[:, ::L1_], -1)

    def gen_excluded():
        return model.generate_next_sem_id(batch, temperature=1, top_k=True, fused=True, sample=False, incremental=True,
                                          constrained=True, exclude_items=seen)

    def gen_model_only():
        hip_ops.beam_candidates, hip_ops.beam_select = stub_candidates, stub_select
        try:
            return model.generate_next_sem_id(batch, temperature=1, top_k=True, fused=True, sample=False)
        finally:
            hip_ops.beam_candidates, hip_ops.beam_select = real

    C, C_full = args.score_candidates, args.score_full_candidates or args.score_candidates
    cands = torch.randint(0, tok.cached_ids.shape[0], (args.batch, max(C, C_full)),
                          generator=torch.Generator().manual_seed(11)).to(device)

    def score(incremental, c):
        return model.score_items(batch, cands[:, :c].contiguous(), incremental=incremental)

    # catalogue filters: about half the corpus allowed — one mask for everyone, and one per user
    gm = torch.Generator().manual_seed(13)
    n_corpus = tok.cached_ids.shape[0]
    shared_mask = (torch.rand(n_corpus, generator=gm) < 0.5).to(device)
    user_masks = (torch.rand(args.batch, n_corpus, generator=gm) < 0.5).to(device)
    shared_filter, user_filter = tok.item_filter(shared_mask), tok.item_filter(user_masks)
    own_group = torch.arange(args.batch, device=device)
    # score bias: 2 randn per item — one table for everyone, and one per user for the builder's time
    shared_table = (2.0 * torch.randn(n_corpus, generator=gm)).to(device)
    user_tables = (2.0 * torch.randn(args.batch, n_corpus, generator=gm)).to(device)
    shared_bias = tok.item_bias(shared_table)

    top = gen(True).sem_ids.contiguous()
    actual = batch.sem_ids_fut.contiguous()
    top[::3, 4] = actual[::3]          # some hits, as a trained model has
    acc = TopKAccumulator(ks=[1, 5, 10])

    def acc_device():
        acc.accumulate(actual=actual, top_k=top)

    def acc_reference():
        reference_accumulate({}, [1, 5, 10], actual, top)

    forms = {"unfused": lambda: gen(False), "fused": lambda: gen(True),
             "incremental": lambda: gen(True, True), "constrained": gen_constrained, "excluded": gen_excluded,
             "model": gen_model_only,
             "acc_device": acc_device, "acc_reference": acc_reference,
             "recommend": lambda: model.recommend(batch, k=10), "score": lambda: score(True, C),
             "score_full": lambda: score(False, C_full),
             "wide": lambda: model.recommend(batch, k=min(100, args.beams), beams=args.beams),
             "wide_excluded": lambda: model.recommend(batch, k=min(100, args.beams), beams=args.beams,
                                                      exclude_items=seen),
             "recommend_forced": recommend_forced, "sampled_items": lambda: model.sample_items(batch, k=10),
             "filtered_shared": lambda: model.recommend(batch, k=10, item_filter=shared_filter),
             "filtered_groups": lambda: model.recommend(batch, k=10, item_filter=user_filter, filter_group=own_group),
             "filter_build": lambda: tok.item_filter(shared_mask),
             "filter_build_groups": lambda: tok.item_filter(user_masks),
             "biased": lambda: model.recommend(batch, k=10, item_bias=shared_bias),
             "bias_build": lambda: tok.item_bias(shared_table),
             "bias_build_groups": lambda: tok.item_bias(user_tables)}
    if args.only:
        forms = {args.only: forms[args.only]}
    elif args.forms:
        forms = {n: forms[n] for n in args.forms}
    times = {n: [] for n in forms}
    for rep in range(-args.warmup, args.reps):
        for name, fn in forms.items():   # alternating: every form sees the same drift of the shared host
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if rep >= 0:
                times[name].append((time.perf_counter() - t0) * 1e3)
    med = {n: statistics.median(v) for n, v in times.items() if v}
    out = {"shape": dict(B=B, k=k, n_cand=n_cand, V=256, L1=L1), "reps": args.reps,
           "median_ms": {n: round(v, 4) for n, v in med.items()},
           "min_max_ms": {n: [round(min(v), 4), round(max(v), 4)] for n, v in times.items() if v}}
    peak = {}
    for name in ("unfused", "fused", "incremental", "constrained", "excluded", "recommend", "score", "score_full",
                 "wide", "wide_excluded", "recommend_forced", "sampled_items", "filtered_shared", "filtered_groups",
                 "biased"):
        if name in forms and not args.only:   # one more call of each generation form, alone after a peak reset
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats(device)
            forms[name]()
            torch.cuda.synchronize()
            peak[name] = round(torch.cuda.max_memory_allocated(device) / 2 ** 20, 1)
    if peak:
        out["peak_mem_mib"] = peak
    if {"fused", "incremental"} <= set(med):
        out["incremental_speedup"] = round(med["fused"] / med["incremental"], 4)
    if {"incremental", "constrained"} <= set(med):
        # the acceptance condition: the constrained form's median within the incremental form's own spread
        spread = max(times["incremental"]) - min(times["incremental"])
        out["constrained_vs_incremental"] = dict(delta_ms=round(med["constrained"] - med["incremental"], 4),
                                                 incremental_spread_ms=round(spread, 4),
                                                 within_spread=med["constrained"] - med["incremental"] <= spread)
    if {"constrained", "excluded"} <= set(med):
        # the exclusion's cost against the constrained form of the same run, next to that form's own spread
        spread = max(times["constrained"]) - min(times["constrained"])
        out["excluded_vs_constrained"] = dict(delta_ms=round(med["excluded"] - med["constrained"], 4),
                                              constrained_spread_ms=round(spread, 4), history=n_hist,
                                              within_spread=med["excluded"] - med["constrained"] <= spread)
    if "recommend" in med and {"filtered_shared", "filtered_groups"} & set(med):
        # the yardstick is the unfiltered call of the same run: the ratio, next to that call's own spread
        lo, hi = min(times["recommend"]), max(times["recommend"])
        out["filtered_vs_recommend"] = dict(
            ratio={n: round(med[n] / med["recommend"], 4) for n in ("filtered_shared", "filtered_groups") if n in med},
            recommend_min_max_over_median=[round(lo / med["recommend"], 4), round(hi / med["recommend"], 4)],
            groups=dict(filtered_shared=1, filtered_groups=args.batch), allowed_fraction=0.5)
    if {"constrained", "biased"} <= set(med):
        # the yardstick is the unbiased constrained search of the same run: the ratio, next to that form's own spread
        lo, hi = min(times["constrained"]), max(times["constrained"])
        out["biased_vs_constrained"] = dict(
            ratio=round(med["biased"] / med["constrained"], 4), delta_ms=round(med["biased"] - med["constrained"], 4),
            constrained_min_max_over_median=[round(lo / med["constrained"], 4), round(hi / med["constrained"], 4)],
            groups=1)
    if {"bias_build", "bias_build_groups"} & set(med):
        out["bias_build"] = dict(items=n_corpus, groups=dict(bias_build=1, bias_build_groups=args.batch))
    if {"wide", "wide_excluded"} & set(med):
        out["wide"] = dict(beams=args.beams, k=min(100, args.beams))
    if {"score", "score_full"} & set(med):
        out["score_candidates"] = {n: c for n, c in (("score", C), ("score_full", C_full)) if n in med}
    if {"unfused", "fused", "model"} <= set(med):
        out["beam_logic_share"] = {n: round(1 - med["model"] / med[n], 4) for n in ("unfused", "fused")}
        out["beam_logic_ms"] = {n: round(med[n] - med["model"], 4) for n in ("unfused", "fused")}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
