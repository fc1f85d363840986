// Decoder evaluation on the device: the per-step beam logic of generate_next_sem_id (reference
// modules/model.py:176-201) in two launches, and the Hit@k counters of evaluate/metrics.py:15-28.
//
//   beam_candidates_kernel  one wave per logits row: softmax(logits / T), optional Exponential(1) noise
//                           (score p / noise: the n_cand largest are a draw of multinomial without
//                           replacement), the n_cand best classes by rank counting out of LDS.
//   beam_select_kernel      one workgroup per batch element: prefix verification (a caller-provided mask or
//                           a binary search of the tokenizer's packed-prefix table), the cumulative score,
//                           the k best of the kprev * n_cand candidates in stable order, the parent gather.
//   beam_expand_kernel      constrained decoding, the whole beam step in one launch: one workgroup per batch
//                           element walks the corpus' prefix trie (only valid continuations are scored), the k
//                           best in stable order, the parent gather and each winner's trie node. A second
//                           instantiation (BLOCKED) skips the children found in a per-user sorted row of blocked
//                           nodes (seen-item exclusion); FILTERED keeps only the children whose bit is set in the
//                           user's row of a per-group node bitmap (catalogue filters), read from global memory;
//                           BIASED ranks by log p + the user's row of per-group subtree bounds (per-item score bias)
//                           and writes the unbiased log p beside the ranking score.
//   beam_expand_wide_kernel the same step for up to 1,024 beams in and out, any kprev * V: the candidates are enumerated
//                           from the trie instead of kept as a dense key array, the k best come from an exact radix
//                           select and one LDS sort; bit for bit beam_expand_kernel's outputs where both take the shape.
//   beam_expand_sampled_kernel  beam_expand_kernel's step for stochastic beam search: the k best by Gumbel-perturbed
//                           score (the caller's Exponential(1) noise, top-down max conditioning) — after the last level
//                           a draw of k corpus rows without replacement.
//   score_paths_kernel     teacher-forced scoring of caller-named candidates: one workgroup per user, per step the
//                           log-probability of every candidate's token in beam_expand_kernel's arithmetic (bitwise),
//                           accumulated over the steps; on the last step each candidate's rank among the user's.
//   trie_blocked_kernel     one workgroup per user: the trie nodes of every level whose leaves are all on the
//                           user's exclusion list, sorted / deduplicated / counted in LDS.
//   trie_allowed_kernel     catalogue filters: per group of an item mask the bitmap of every level's nodes with an
//                           allowed item below them (bit OR) and every leaf's lowest allowed item (index MIN).
//   trie_bias_kernel        per-item score bias: per group of a bias table every level's per-node maximum of the items
//                           below (the bound the biased expand adds) and every leaf's item that attains it.
//   beam_self_attn_kernel   incremental decoding: the newest token's causal self-attention over its beam's
//                           ancestors, read in place from every step's packed qkv output through an
//                           ancestor row table (no per-beam cache is gathered or appended).
//   topk_hits_kernel        one wave per batch row: first matching beam rank per sem-ID slice / position,
//                           counters accumulated on the device with one atomic per (wave, counter).
//   rank_hist_kernel        one wave per batch row: the rank of the first beam equal to the target in every column,
//                           a workgroup-local histogram, one atomic per non-empty bin.
#include <float.h>

#include <type_traits>

#include "common.h"

namespace rqhip {

constexpr int kBeamMaxV = 4096;
constexpr int kBeamMaxN = 8192;
constexpr int kHitsMaxD = 64;
constexpr int kHitsMaxKs = 8;
constexpr int kNoRank = 0x7fffffff;   // no beam matched
constexpr int kBlockedMax = 1024;     // widest blocked row / exclusion list
constexpr int kRankMaxK = 1024;

// ------------------------------------------------------------------------------------- candidates
// (max, lowest index of the max) over the wave; NaN never wins a comparison, so a row with a NaN keeps the
// max of its other entries (its NaN entries then score lowest, below).
__device__ __forceinline__ void wave_argmax(float& m, int& idx) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const float om = __shfl_xor(m, o, 64);
    const int oi = __shfl_xor(idx, o, 64);
    if (om > m || (om == m && oi < idx)) { m = om; idx = oi; }
  }
}

// The classes a lane owns, ascending: f(j, v) for v = lane + 64 j < V. J > 0: J unrolled steps (j is a constant in
// each, so a row can live in J registers per lane); J == 0: as many steps as V needs.
template <int J, typename F>
__device__ __forceinline__ void for_owned(int V, int lane, F f) {
  if constexpr (J > 0) {
#pragma unroll
    for (int j = 0; j < J; ++j) {
      const int v = lane + 64 * j;
      if (v < V) f(j, v);
    }
  } else {
    for (int v = lane, j = 0; v < V; v += 64, ++j) f(j, v);
  }
}

// Softmax statistics of one row z = logits / T, formed by one wave: the max, then the sum of the other classes'
// exp(z - max) — the max class (its lowest index) contributes exactly 1, so log p = (z - max) - log1p(rest) keeps full
// relative precision where one class dominates (log p -> -rest, not log(1.0f) = 0).
struct RowStats {
  float m, sum, log_norm;   // max z; 1 + rest; log1p(rest)
};
// Where a kernel keeps its row is its own business: load(j, v) gives z of class v, shifted(j, v, m) gives z - m
// (for_owned's (j, v); each is called once per owned class, loads first). Every kernel's statistics come from this one
// sequence of operations, so equal rows give equal bits in all of them.
template <int J, typename Load, typename Shifted>
__device__ __forceinline__ RowStats row_stats(int V, int lane, Load load, Shifted shifted) {
  float m = -INFINITY;
  int am = 0x7fffffff;
  for_owned<J>(V, lane, [&](int j, int v) {
    const float z = load(j, v);
    if (z > m) { m = z; am = v; }
  });
  wave_argmax(m, am);
  float rest = 0.f;
  for_owned<J>(V, lane, [&](int j, int v) {
    const float dv = shifted(j, v, m);
    if (v != am) rest += expf(dv);
  });
  rest = group_sum<64>(rest);
  return {m, rest + 1.0f, log1pf(rest)};
}
// log softmax of the class with dv = z - max; -inf where its probability underflows to 0
__device__ __forceinline__ float log_prob(float dv, const RowStats& st) {
  const float p = expf(dv) / st.sum;
  return p == 0.f ? -INFINITY : dv - st.log_norm;
}

// First index in [lo, hi) of the ascending a[] (global or LDS) whose entry is >= key (lower_bound) / > key
// (upper_bound); hi if there is none.
template <typename T, typename I>
__device__ __forceinline__ I lower_bound(const T* a, I lo, I hi, T key) {
  while (lo < hi) {
    const I mid = (lo + hi) >> 1;
    if (a[mid] < key) lo = mid + 1; else hi = mid;
  }
  return lo;
}
template <typename T, typename I>
__device__ __forceinline__ I upper_bound(const T* a, I lo, I hi, T key) {
  while (lo < hi) {
    const I mid = (lo + hi) >> 1;
    if (a[mid] <= key) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// LDS per wave: d[Vp] (z - max, the log of the unnormalised probability) then s[Vp] (the scores), Vp = V
// rounded up to 4. Every lane owns the classes v = lane + 64 j.
__global__ void __launch_bounds__(256) beam_candidates_kernel(const float* __restrict__ logits,
                                                              const float* __restrict__ noise, int64_t R, int V,
                                                              int Vp, int n_cand, float temperature,
                                                              int64_t* __restrict__ cand_ids,
                                                              float* __restrict__ cand_lp) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
  float* d = reinterpret_cast<float*>(smem) + (size_t)wave * 2 * Vp;
  float* s = d + Vp;
  const int64_t row_raw = (int64_t)blockIdx.x * waves + wave;
  const bool live = row_raw < R;
  const int64_t row = live ? row_raw : R - 1;   // idle waves repeat the last row (uniform barriers), write nothing
  const float* x = logits + row * V;

  const RowStats st = row_stats<0>(
      V, lane, [&](int, int v) { return d[v] = x[v] / temperature; },
      [&](int, int v, float m) { return d[v] = d[v] - m; });
  for (int v = lane; v < Vp; v += 64) {
    float sc = -2.0f;   // padding: below every real score
    if (v < V) {
      const float p = expf(d[v]) / st.sum;
      sc = noise ? p / noise[row * V + v] : p;
      if (!(sc == sc)) sc = -1.0f;   // NaN (a NaN logit, 0 / 0): ranked last, ties by index — ranks stay a permutation
    }
    s[v] = sc;
  }
  __syncthreads();
  const float4* s4 = reinterpret_cast<const float4*>(s);
  for (int v0 = lane; v0 < V; v0 += 256) {
    float sv[4];
    int vi[4], cnt[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      vi[j] = v0 + 64 * j;
      sv[j] = vi[j] < V ? s[vi[j]] : INFINITY;
      cnt[j] = 0;
    }
    for (int u4 = 0; u4 < Vp / 4; ++u4) {
      const float4 q = s4[u4];
      const float su[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int u = 4 * u4 + t;
#pragma unroll
        for (int j = 0; j < 4; ++j) cnt[j] += (su[t] > sv[j]) || (su[t] == sv[j] && u < vi[j]);
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (live && vi[j] < V && cnt[j] < n_cand) {
        cand_ids[row * n_cand + cnt[j]] = vi[j];
        cand_lp[row * n_cand + cnt[j]] = log_prob(d[vi[j]], st);
      }
    }
  }
}

// ------------------------------------------------------------------------------------- select
// float -> uint32 whose unsigned order is the float order (NaN on top, as torch.sort(descending) places
// it); 0 is below every float's key and marks a taken candidate.
__device__ __forceinline__ uint32_t score_key(float f) {
  if (f != f) return 0xFFFFFFFFu;
  const uint32_t b = __builtin_bit_cast(uint32_t, f);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float key_score(uint32_t k) {
  if (k == 0xFFFFFFFFu) return NAN;
  return __builtin_bit_cast(float, (k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
}
// best = larger key, then lower candidate index
__device__ __forceinline__ bool better(uint32_t ka, int ia, uint32_t kb, int ib) {
  return ka > kb || (ka == kb && ia < ib);
}

constexpr int kSelThreads = 256;

// Selection: k rounds of a workgroup argmax over key[0, N) in LDS (0 = absent or taken). A thread owns the
// candidates e = tid + nthr j and keeps the best of them cached; a round is one wave reduction, an exchange of the
// waves' winners through LDS (lanes 0..nwave-1 pick them up: a butterfly inside the first MAXW lanes, lane 0
// broadcasts), and a rescan by the single thread that owned the winner — about k (12 shuffles + the exchange + 2
// barriers + 32 LDS reads) for k = 32, N = 6400 on 256 threads, against N log^2 N / 256 ~ 2000 compare-exchange
// steps with a barrier each for an LDS bitonic sort of 8192 keys. out(r, wk, wi) runs on every thread with round r's
// winner, best first in better()'s order; wk == 0 (block-uniform): no candidate is left, in this round or later.
// LDS behind key[]: at N rounded up to 4 the waves' keys [MAXW], then their indices [MAXW]. nthr = blockDim.x, a
// multiple of 64 up to 64 MAXW. A thread reads only its own entries of key[] here: the caller needs a barrier before
// the call only where other threads wrote them.
template <int MAXW, typename Out>
__device__ __forceinline__ void select_rounds(uint32_t* key, int N, int k, int nthr, Out out) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nwave = nthr >> 6;
  uint32_t* w_key = key + (N + 3) / 4 * 4;
  int* w_idx = reinterpret_cast<int*>(w_key + MAXW);
  uint32_t best_k;
  int best_i;
  auto scan_own = [&] {
    best_k = 0;
    best_i = 0x7fffffff;
    for (int e = tid; e < N; e += nthr) {
      const uint32_t kk = key[e];
      if (better(kk, e, best_k, best_i)) { best_k = kk; best_i = e; }
    }
  };
  scan_own();
  for (int r = 0; r < k; ++r) {
    uint32_t wk = best_k;
    int wi = best_i;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
      const uint32_t ok_ = __shfl_xor(wk, o, 64);
      const int oi = __shfl_xor(wi, o, 64);
      if (better(ok_, oi, wk, wi)) { wk = ok_; wi = oi; }
    }
    if (lane == 0) { w_key[wave] = wk; w_idx[wave] = wi; }
    __syncthreads();
    wk = lane < nwave ? w_key[lane] : 0;
    wi = lane < nwave ? w_idx[lane] : 0x7fffffff;
#pragma unroll
    for (int o = MAXW / 2; o >= 1; o >>= 1) {
      const uint32_t ok_ = __shfl_xor(wk, o, 64);
      const int oi = __shfl_xor(wi, o, 64);
      if (better(ok_, oi, wk, wi)) { wk = ok_; wi = oi; }
    }
    wk = __shfl(wk, 0, 64);
    wi = __shfl(wi, 0, 64);
    __syncthreads();   // w_key / w_idx are rewritten next round
    if (wk != 0 && tid == (wi % nthr)) {
      key[wi] = 0;
      scan_own();
    }
    out(r, wk, wi);
  }
}

__global__ void __launch_bounds__(kSelThreads) beam_select_kernel(
    const int64_t* __restrict__ cand_ids, const float* __restrict__ cand_lp, const bool* __restrict__ valid,
    const int64_t* __restrict__ keys, int64_t n_keys, int64_t base, int64_t checked,
    const int64_t* __restrict__ parents, const float* __restrict__ parent_lp, int kprev, int n_cand, int P, int k,
    int64_t* __restrict__ out_ids, float* __restrict__ out_lp, int32_t* __restrict__ out_parent) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x;
  const int N = kprev * n_cand;
  uint32_t* key = reinterpret_cast<uint32_t*>(smem);   // [N rounded up to 4], then select_rounds' exchange
  const int64_t b = blockIdx.x;
  const int64_t* cid = cand_ids + b * N;
  const float* clp = cand_lp + b * N;

  for (int e = tid; e < N; e += kSelThreads) {
    const int par = e / n_cand;
    const int64_t c = cid[e];
    bool ok;
    if (valid) {
      ok = valid[b * N + e];
    } else {
      // (parent prefix, candidate) packed in base `base` as semids._pack; every element must be a digit
      const int64_t* pp = parents + (b * kprev + par) * P;
      int64_t q = 0;
      ok = c >= 0 && c < base && b * N + e < checked && n_keys > 0;
      for (int j = 0; j < P; ++j) {
        const int64_t t = pp[j];
        ok = ok && t >= 0 && t < base;
        q = q * base + t;
      }
      q = q * base + c;
      if (ok) {
        const int64_t at = lower_bound(keys, (int64_t)0, n_keys, q);
        ok = at < n_keys && keys[at] == q;
      }
    }
    const float sc = ((ok ? 0.0f : -10000.0f) + clp[e]) + (parent_lp ? parent_lp[b * kprev + par] : 0.0f);
    key[e] = score_key(sc);   // never 0
  }
  // k <= N: every round finds an untaken candidate (wk != 0, wi < N)
  select_rounds<kSelThreads / 64>(key, N, k, kSelThreads, [&](int r, uint32_t wk, int wi) {
    if (tid == 0) {
      out_lp[b * k + r] = key_score(wk);
      if (out_parent) out_parent[b * k + r] = wi / n_cand;
    }
    // the winner's row: parent prefix then the candidate id
    int64_t* o = out_ids + (b * k + r) * (P + 1);
    if (tid < P) o[tid] = parents[(b * kprev + wi / n_cand) * P + tid];   // P < 64
    if (tid == 0) o[P] = cid[wi];
  });
}

// ------------------------------------------------------------------------------------- expand (trie walk)
// Constrained beam step: one workgroup per batch element walks the corpus' prefix trie instead of drawing,
// searching and masking candidates. The candidates of beam j are the children of its level-P node — a contiguous
// range of level P + 1 that ascends by token — so only real continuations are ever scored.
//   1. a wave per beam (round robin; 16 waves when kprev > 4, else 4: a beam is a chain of dependent global loads
//      — node, child range, logits row, tokens — so this phase is latency-bound and more waves are what hides it):
//      the row's statistics by row_stats and log p by log_prob, the functions beam_candidates_kernel uses, so log p
//      is bitwise what that kernel returns; the same wave then walks the node's children and writes
//      score_key(log p + parent_lp) to key[j V + token] in LDS (0 = absent: the (beam, token) tie rule is the index
//      order).
//   2. select_rounds over key[], as in beam_select_kernel; a round that finds only absent entries writes a dead row
//      (ids -1, -inf, parent 0, node -1), as do all rounds after it.
//   3. each winner's node index: a binary search of its parent's child range (<= 12 dependent probes), one
//      thread per output row after the rounds, so the probes of the k rows overlap instead of stalling a round each.
// Tables are the caller's contract but never trusted for addressing: node outside [0, n_nodes) is a dead beam,
// child_off is clamped into [0, n_children], tokens outside [0, V) are skipped.
// BLOCKED: `blocked` (B, n_blocked) int32 holds per user the level-(P + 1) nodes that are not candidates, ascending
// and INT32_MAX-padded; the row is staged once into LDS after the exchange area and phase 1 looks every child index
// up in it (a binary search over [0, n_blocked): an unsorted row filters the wrong children, never reads outside).
// FILTERED: `allowed` holds G rows of n_words words, bit (c & 31) of word (c >> 5) set iff the level-(P + 1) node c has
// an allowed item below it in that group; batch element b reads row group[b], or is unfiltered when group[b] is outside
// [0, G). The rows stay in global memory (a level's row is a few KB at most, shared by the users of a group and
// L2-resident): the LDS layout does not grow. A word outside [0, n_words) reads as "not allowed". Both filters may be
// given: a candidate passes both.
constexpr int kExpMaxWaves = 16;

struct AllowedBits {   // FILTERED's arguments; never read otherwise
  const int32_t* bits;    // (G, n_words)
  const int32_t* group;   // (B)
  int n_words, G;
};
struct BiasArgs {   // BIASED's arguments, in AllowedBits' place
  const float* rows;      // (G, n_bias): the level-(P + 1) subtree bounds
  const int32_t* group;   // (B), or NULL: nobody is biased
  int n_bias, G;
  float* out_score;       // (B, k): the ranking key; out_lp then carries the unbiased log p
};
template <bool BIASED>
using ChildRows = std::conditional_t<BIASED, BiasArgs, AllowedBits>;

// A bias value as every kernel reads it: NaN and +inf are -inf (a bad value can only hide an item), -0.0 is +0.0
__device__ __forceinline__ float clean_bias(float u) {
  if (u != u || u == INFINITY) return -INFINITY;
  return u == 0.0f ? 0.0f : u;
}

// One level of the trie: the nodes' child offsets and the next level's tokens, as the caller passed them.
struct TrieLevel {
  const int32_t* __restrict__ child_off;
  int n_nodes;
  const int32_t* __restrict__ tok;
  int n_children;
  // node nd's child range [lo, hi), clamped into [0, n_children]; false (no range) for a node outside [0, n_nodes)
  __device__ __forceinline__ bool children(int nd, int& lo, int& hi) const {
    if (nd < 0 || nd >= n_nodes) return false;
    lo = min(max(child_off[nd], 0), n_children);
    hi = min(max(child_off[nd + 1], 0), n_children);
    return true;
  }
};

// One user's filters on a level's children: which of them are candidates, and what is added to a candidate's score,
// is stated here and nowhere else.
struct ChildFilter {
  const int* blk;        // BLOCKED: the user's blocked row, staged in LDS
  int n_blocked;
  const int32_t* arow;   // FILTERED: the user's bitmap row (global memory)
  int n_words;           // < 0: the user is not filtered
  const float* brow;     // BIASED: the user's row of subtree bounds (global memory)
  int n_bias;            // < 0: the user is not biased
  // c >= 0, a child index: it has an allowed item below it
  template <bool BLOCKED, bool FILTERED>
  __device__ __forceinline__ bool allowed(int c) const {
    if constexpr (FILTERED) {
      if (n_words < 0) return true;
      const int w = c >> 5;
      return w < n_words && (((uint32_t)arow[w] >> (c & 31)) & 1u);
    }
    return true;
  }
  // child c with token v is a candidate: a class the model can generate (not e.g. a dedup count >= V), not every leaf
  // below it excluded for the user, an allowed item below it
  template <bool BLOCKED, bool FILTERED>
  __device__ __forceinline__ bool candidate(int c, int v, int V) const {
    if (v < 0 || v >= V) return false;
    if constexpr (BLOCKED) {
      const int at = lower_bound(blk, 0, n_blocked, c);
      if (at < n_blocked && blk[at] == c) return false;
    }
    return allowed<BLOCKED, FILTERED>(c);
  }
  // BIASED: the above, and for a biased user a bound above -inf (some item below c may still be shown); add = the
  // bound, read once (an index outside [0, n_bias) reads as -inf and is never read)
  template <bool BLOCKED, bool FILTERED, bool BIASED>
  __device__ __forceinline__ bool candidate(int c, int v, int V, float& add) const {
    static_assert(!(FILTERED && BIASED), "a filter is written into the bias as -inf");
    add = 0.0f;
    if (!candidate<BLOCKED, FILTERED>(c, v, V)) return false;
    if constexpr (BIASED) {
      if (n_bias < 0) return true;
      add = c < n_bias ? clean_bias(brow[c]) : -INFINITY;
      return add > -INFINITY;
    }
    return true;
  }
  // the ranking score of a candidate with log-probability lp: one add for a biased user, lp itself otherwise
  template <bool BIASED>
  __device__ __forceinline__ float score(float lp, float add) const {
    if constexpr (BIASED) {
      if (n_bias >= 0) return lp + add;
    }
    return lp;
  }
};
// batch element b's filters over the staged row blk; a group outside [0, G) leaves b unfiltered / unbiased
template <bool FILTERED>
__device__ __forceinline__ ChildFilter child_filter(const int* blk, int n_blocked, const AllowedBits& a, int64_t b) {
  ChildFilter f = {blk, n_blocked, nullptr, -1, nullptr, -1};
  if constexpr (FILTERED) {
    const int g = a.group[b];
    if (g >= 0 && g < a.G) {
      f.arow = a.bits + (int64_t)g * a.n_words;
      f.n_words = a.n_words;
    }
  }
  return f;
}
template <bool FILTERED>
__device__ __forceinline__ ChildFilter child_filter(const int* blk, int n_blocked, const BiasArgs& a, int64_t b) {
  ChildFilter f = {blk, n_blocked, nullptr, -1, nullptr, -1};
  const int g = a.group ? a.group[b] : -1;
  if (g >= 0 && g < a.G) {
    f.brow = a.rows + (int64_t)g * a.n_bias;
    f.n_bias = a.n_bias;
  }
  return f;
}

// The dense kernels' LDS: key[N rounded up to 4], select_rounds' exchange, then (BLOCKED)
// blk[n_blocked <= kBlockedMax], then (BIASED) the beams' row statistics m[kprev], sum[kprev], log_norm[kprev]. Zeroes
// key[], stages batch element b's blocked row and ends on a barrier. Rows: AllowedBits or BiasArgs.
template <bool BLOCKED, bool FILTERED, typename Rows>
__device__ __forceinline__ ChildFilter expand_prologue(char* smem, int N, int64_t b,
                                                       const int32_t* __restrict__ blocked, int n_blocked,
                                                       const Rows& allowed, uint32_t*& key) {
  const int tid = threadIdx.x, nthr = blockDim.x;
  key = reinterpret_cast<uint32_t*>(smem);
  int* blk = reinterpret_cast<int*>(key + (N + 3) / 4 * 4 + 2 * kExpMaxWaves);
  for (int e = tid; e < N; e += nthr) key[e] = 0;
  if constexpr (BLOCKED) {
    for (int e = tid; e < n_blocked; e += nthr) blk[e] = blocked[b * n_blocked + e];
  }
  __syncthreads();
  return child_filter<FILTERED>(blk, n_blocked, allowed, b);
}

// A dense kernel's output rows of batch element b, (k) each: beam 0 of the user is row 0 of every array here.
struct ExpandRows {
  int64_t* ids;      // (k, P + 1)
  float* score;      // the selection's score: key_score of the winner's key
  float* later;      // sampled: out_phi, biased: out_lp — -inf in a dead row and written after the rounds in a live
                     // one; else NULL
  int32_t* parent;
  int32_t* node;
};
// select_rounds' out() of the dense kernels: round r's row — dead (ids -1, -inf, parent 0, node -1) when no candidate
// is left, else the parent's prefix, the token, the score and the parent's index; its node follows in expand_nodes.
__device__ __forceinline__ void expand_write_row(const ExpandRows& o, int r, uint32_t wk, int wi,
                                                 const int64_t* __restrict__ parents, int V, int P) {
  const int tid = threadIdx.x;
  int64_t* row = o.ids + (int64_t)r * (P + 1);
  if (wk == 0) {   // no candidate left: a dead row
    if (tid <= P) row[tid] = -1;   // P < 64
    if (tid == 0) {
      if (o.later) o.later[r] = -INFINITY;
      o.score[r] = -INFINITY;
      o.parent[r] = 0;
      o.node[r] = -1;
    }
    return;
  }
  const int par = wi / V, v = wi - par * V;
  if (tid < P) row[tid] = parents[(int64_t)par * P + tid];
  if (tid == 0) {
    row[P] = v;
    o.score[r] = key_score(wk);
    o.parent[r] = par;
  }
}
// After the rounds, a thread per row: the winner's node, the child of its parent's node (nd0[parent], the root without
// nd0) that carries its token — the first entry >= v of the node's ascending range; -1: an unsorted (bad) table.
// live(r, v): whatever else the same thread owes a live row r with token v.
template <typename Live>
__device__ __forceinline__ void expand_nodes(const ExpandRows& o, int k, int P, const int32_t* __restrict__ nd0,
                                             const TrieLevel& lvl, Live live) {
  __syncthreads();   // thread 0's rows (global) are visible to the workgroup
  for (int r = threadIdx.x; r < k; r += blockDim.x) {
    const int v = (int)o.ids[(int64_t)r * (P + 1) + P];
    if (v < 0) continue;   // a dead row: its node is already -1
    int lo, hi, at = -1;
    if (lvl.children(nd0 ? nd0[o.parent[r]] : 0, lo, hi)) {
      at = lower_bound(lvl.tok, lo, hi, v);
      if (!(at < hi && lvl.tok[at] == v)) at = -1;
    }
    o.node[r] = at;
    live(r, v);
  }
}
__device__ __forceinline__ void expand_nodes(const ExpandRows& o, int k, int P, const int32_t* __restrict__ nd0,
                                             const TrieLevel& lvl) {
  expand_nodes(o, k, P, nd0, lvl, [](int, int) {});
}

// BIASED: the ranking key of a candidate is s = lp + the bound of its subtree (ChildFilter::score), so the k best are
// the k best by what a completion of the prefix can still score; rows.score is then out_score and out_lp, the unbiased
// lp that the next step adds to, is formed again after the rounds by expand_nodes' thread from the parent beam's
// statistics, which phase 1 leaves in LDS (three floats per beam behind the blocked row): the operations of phase 1,
// the same bits. Only this form grows the LDS layout and takes kprev <= kWideMax (the host refuses more).
template <bool BLOCKED, bool FILTERED, bool BIASED = false>
__global__ void __launch_bounds__(64 * kExpMaxWaves) beam_expand_kernel(
    const float* __restrict__ logits, float temperature, const int32_t* __restrict__ node, TrieLevel lvl,
    const int64_t* __restrict__ parents, const float* __restrict__ parent_lp, int kprev, int V, int P, int k,
    int64_t* __restrict__ out_ids, float* __restrict__ out_lp, int32_t* __restrict__ out_parent,
    int32_t* __restrict__ out_node, const int32_t* __restrict__ blocked, int n_blocked, ChildRows<BIASED> allowed) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nthr = blockDim.x, nwave = nthr >> 6;   // 4 or kExpMaxWaves waves (the host picks by kprev)
  const int N = kprev * V;
  const int64_t b = blockIdx.x;
  const int32_t* nd0 = node ? node + b * kprev : nullptr;
  uint32_t* key;
  const ChildFilter flt = expand_prologue<BLOCKED, FILTERED>(smem, N, b, blocked, n_blocked, allowed, key);
  // BIASED: m[kprev], sum[kprev], log_norm[kprev] behind the blocked row
  float* stat = reinterpret_cast<float*>(key + (N + 3) / 4 * 4 + 2 * kExpMaxWaves) + (BLOCKED ? n_blocked : 0);

  for (int j = wave; j < kprev; j += nwave) {
    int lo, hi;
    if (!lvl.children(nd0 ? nd0[j] : 0, lo, hi) || lo >= hi) continue;   // dead beam (wave-uniform)
    const float* x = logits + (b * kprev + j) * V;
    const RowStats st = row_stats<0>(
        V, lane, [&](int, int v) { return x[v] / temperature; },
        [&](int, int v, float m) { return x[v] / temperature - m; });
    const float plp = parent_lp ? parent_lp[b * kprev + j] : 0.0f;
    if constexpr (BIASED) {
      if (lane == 0) { stat[j] = st.m; stat[kprev + j] = st.sum; stat[2 * kprev + j] = st.log_norm; }
      for (int c = lo + lane; c < hi; c += 64) {
        const int v = lvl.tok[c];
        float add;
        if (!flt.candidate<BLOCKED, FILTERED, BIASED>(c, v, V, add)) continue;
        key[j * V + v] = score_key(flt.score<BIASED>(log_prob(x[v] / temperature - st.m, st) + plp, add));
      }
    } else {
      for (int c = lo + lane; c < hi; c += 64) {
        const int v = lvl.tok[c];
        if (!flt.candidate<BLOCKED, FILTERED>(c, v, V)) continue;
        key[j * V + v] = score_key(log_prob(x[v] / temperature - st.m, st) + plp);
      }
    }
  }
  __syncthreads();

  if constexpr (BIASED) {
    const ExpandRows rows = {out_ids + b * k * (P + 1), allowed.out_score + b * k, out_lp + b * k, out_parent + b * k,
                             out_node + b * k};
    select_rounds<kExpMaxWaves>(key, N, k, nthr, [&](int r, uint32_t wk, int wi) {
      expand_write_row(rows, r, wk, wi, parents + b * kprev * P, V, P);
    });
    expand_nodes(rows, k, P, nd0, lvl, [&](int r, int v) {
      const int j = rows.parent[r];   // a live row: a beam that phase 1 scored
      const RowStats st = {stat[j], stat[kprev + j], stat[2 * kprev + j]};
      const float plp = parent_lp ? parent_lp[b * kprev + j] : 0.0f;
      rows.later[r] = log_prob(logits[(b * kprev + j) * V + v] / temperature - st.m, st) + plp;
    });
  } else {
    const ExpandRows rows = {out_ids + b * k * (P + 1), out_lp + b * k, nullptr, out_parent + b * k, out_node + b * k};
    select_rounds<kExpMaxWaves>(key, N, k, nthr, [&](int r, uint32_t wk, int wi) {
      expand_write_row(rows, r, wk, wi, parents + b * kprev * P, V, P);
    });
    expand_nodes(rows, k, P, nd0, lvl);
  }
}

// ------------------------------------------------------------------------------------- expand, sampled
// Stochastic beam search (Kool, van Hoof and Welling 2019): beam_expand_kernel's step with the k best taken by
// perturbed score instead of by score, which makes the k leaves after the last step a draw of k items without
// replacement from the trie's own distribution. A beam carries phi (its log-probability under the locally
// renormalised trie distribution) and G (its perturbed score, a Gumbel(phi) value conditioned top-down on the maximum
// of its siblings' subtrees). For a live beam j with (phi_j, G_j) and candidates C_j (its children that
// beam_expand_kernel would score):
//   l_c     = log_prob(...)                        the full-V log-softmax, beam_expand_kernel's bits
//   Lam_j   = max l + log(sum_c exp(l_c - max l))  the candidates' mass: phi must sum to the parent's over C_j, or the
//                                                  truncated-Gumbel step below is not exact
//   phi_c   = phi_j + (l_c - Lam_j)
//   Gt_c    = phi_c - log(e_c)                     e_c the caller's Exponential(1) draw: a Gumbel(phi_c) value
//   Z_j     = max_c Gt_c
//   v       = G_j - Gt_c + log(1 - exp(Gt_c - Z_j))
//   G_c     = G_j - max(v, 0) - log1p(exp(-|v|))   the arg-max child: v = -inf, G_c = G_j exactly
// log(1 - exp(d)) is log(-expm1(d)) for d > -log 2 and log1p(-exp(d)) below (the same quantity, without the
// cancellation of 1 - exp(d) near d = 0). A child with l_c, Lam_j, phi_j or G_j at -inf carries phi_c = G_c = -inf: a
// candidate still, above the absent entries. Phase 1 makes four passes over a beam's children (max l; sum; Gt and its
// max; G), each lane over the same children every time; Gt waits in the child's own key[] slot between the last two.
// key[] then holds score_key(G_c) and the selection is select_rounds, untouched. out_phi is not kept per candidate
// (a second array of kprev V floats does not fit beside key[]): after the rounds a wave per output row forms its
// parent's (statistics, Lam) again with sampled_beam — the one function phase 1 called, so the same bits — and phi_c
// from them. LDS is beam_expand_kernel's.
struct SampledBeam {
  bool live;   // the node is in the level and has a candidate; wave-uniform
  int lo, hi;  // its child range, clamped
  RowStats st;
  float lam, phi, g;
};

// f(c, v) for the candidates among the children [lo, hi) that this lane owns: c = lo + lane + 64 i, v = tok[c]
template <bool BLOCKED, bool FILTERED, typename F>
__device__ __forceinline__ void sampled_for_children(int lo, int hi, int lane, const TrieLevel& lvl, int V,
                                                     const ChildFilter& flt, F f) {
  for (int c = lo + lane; c < hi; c += 64) {
    const int v = lvl.tok[c];
    if (flt.candidate<BLOCKED, FILTERED>(c, v, V)) f(c, v);
  }
}

__device__ __forceinline__ float wave_max(float m) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
  return m;
}

// the position of the n-th set bit of m (n from 0); n >= popcount(m): some position below 64
__device__ __forceinline__ int nth_set_bit(uint64_t m, int n) {
  int pos = 0;
#pragma unroll
  for (int w = 32; w >= 1; w >>= 1) {
    const int cnt = __popcll((unsigned long long)((m >> pos) & ((1ull << w) - 1)));
    if (n >= cnt) { n -= cnt; pos += w; }
  }
  return pos;
}

// Beam j of the user whose beam arrays start at nd0 / phi0 / g0 (NULL on the first step), x its logits row: its child
// range, row statistics and Lam, formed by one wave. Phase 1 and the output phase both call this, for equal bits.
template <bool BLOCKED, bool FILTERED>
__device__ __forceinline__ SampledBeam sampled_beam(int j, int lane, const float* __restrict__ x, float temperature,
                                                    const int32_t* __restrict__ nd0, const TrieLevel& lvl,
                                                    const float* __restrict__ phi0, const float* __restrict__ g0,
                                                    int V, const ChildFilter& flt) {
  SampledBeam s = {false, 0, 0, {0.f, 1.f, 0.f}, -INFINITY, -INFINITY, -INFINITY};
  if (!lvl.children(nd0 ? nd0[j] : 0, s.lo, s.hi) || s.lo >= s.hi) return s;
  s.st = row_stats<0>(
      V, lane, [&](int, int v) { return x[v] / temperature; },
      [&](int, int v, float m) { return x[v] / temperature - m; });
  s.phi = phi0 ? phi0[j] : 0.0f;
  s.g = g0 ? g0[j] : 0.0f;
  float lmax = -INFINITY;
  bool any = false;
  sampled_for_children<BLOCKED, FILTERED>(s.lo, s.hi, lane, lvl, V, flt, [&](int, int v) {
    lmax = fmaxf(lmax, log_prob(x[v] / temperature - s.st.m, s.st));
    any = true;
  });
  if (!__any(any)) return s;
  s.live = true;
  lmax = wave_max(lmax);
  s.lam = -INFINITY;
  if (lmax != -INFINITY) {   // wave-uniform
    float sum = 0.f;
    if constexpr (FILTERED) {
      // The one place where a child's position matters: a lane's partial sum. Here lane t adds the terms of the ALLOWED
      // children of rank t, t + 64, ... among the node's allowed children — the lanes on which the trie of the allowed
      // rows alone holds the same children — so Lam (and with it phi and G) is bitwise that trie's. A child that is
      // allowed but no candidate (blocked, token outside [0, V)) adds 0 on its lane, as it does there. So this is the
      // one caller that asks allowed() apart from candidate(): the first places a child, the second gives its term.
      int before = 0;   // allowed children in the chunks so far
      for (int c0 = s.lo; c0 < s.hi; c0 += 64) {   // wave-uniform
        const int c = c0 + lane;
        const bool in = c < s.hi && flt.allowed<BLOCKED, FILTERED>(c);
        float term = 0.f;
        if (in) {
          const int v = lvl.tok[c];
          if (flt.candidate<BLOCKED, FILTERED>(c, v, V))
            term = expf(log_prob(x[v] / temperature - s.st.m, s.st) - lmax);
        }
        const uint64_t m = __ballot(in);
        const int n = __popcll((unsigned long long)m);
        const int j = (lane - before) & 63;   // this lane takes the chunk's j-th allowed child, if it has one
        const float t = __shfl(term, nth_set_bit(m, j), 64);
        if (j < n) sum += t;
        before += n;
      }
    } else {
      sampled_for_children<BLOCKED, FILTERED>(s.lo, s.hi, lane, lvl, V, flt, [&](int, int v) {
        sum += expf(log_prob(x[v] / temperature - s.st.m, s.st) - lmax);
      });
    }
    s.lam = lmax + logf(group_sum<64>(sum));
  }
  return s;
}

// phi of the child with full-V log-probability l
__device__ __forceinline__ float sampled_child_phi(float l, const SampledBeam& s) {
  if (l == -INFINITY || s.lam == -INFINITY || s.phi == -INFINITY || s.g == -INFINITY) return -INFINITY;
  return s.phi + (l - s.lam);
}

template <bool BLOCKED, bool FILTERED>
__global__ void __launch_bounds__(64 * kExpMaxWaves) beam_expand_sampled_kernel(
    const float* __restrict__ logits, const float* __restrict__ noise, float temperature,
    const int32_t* __restrict__ node, TrieLevel lvl, const int64_t* __restrict__ parents,
    const float* __restrict__ parent_phi, const float* __restrict__ parent_g, int kprev, int V, int P, int k,
    int64_t* __restrict__ out_ids, float* __restrict__ out_phi, float* __restrict__ out_g,
    int32_t* __restrict__ out_parent, int32_t* __restrict__ out_node, const int32_t* __restrict__ blocked,
    int n_blocked, AllowedBits allowed) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nthr = blockDim.x, nwave = nthr >> 6;   // 4 or kExpMaxWaves waves (the host picks by kprev)
  const int N = kprev * V;
  const int64_t b = blockIdx.x;
  const int32_t* nd0 = node ? node + b * kprev : nullptr;
  const float* phi0 = parent_phi ? parent_phi + b * kprev : nullptr;
  const float* g0 = parent_g ? parent_g + b * kprev : nullptr;
  uint32_t* key;
  const ChildFilter flt = expand_prologue<BLOCKED, FILTERED>(smem, N, b, blocked, n_blocked, allowed, key);

  for (int j = wave; j < kprev; j += nwave) {
    const float* x = logits + (b * kprev + j) * V;
    const SampledBeam s = sampled_beam<BLOCKED, FILTERED>(j, lane, x, temperature, nd0, lvl, phi0, g0, V, flt);
    if (!s.live) continue;   // wave-uniform
    const float* e = noise + (b * kprev + j) * V;
    float z = -INFINITY;
    sampled_for_children<BLOCKED, FILTERED>(s.lo, s.hi, lane, lvl, V, flt, [&](int, int v) {
      const float pc = sampled_child_phi(log_prob(x[v] / temperature - s.st.m, s.st), s);
      float ev = e[v];
      if (!(ev > 0.f && ev <= FLT_MAX)) ev = FLT_MIN;
      const float gt = pc - logf(ev);   // -inf with pc
      key[j * V + v] = __builtin_bit_cast(uint32_t, gt);
      z = fmaxf(z, gt);
    });
    z = wave_max(z);
    sampled_for_children<BLOCKED, FILTERED>(s.lo, s.hi, lane, lvl, V, flt, [&](int, int v) {
      const float gt = __builtin_bit_cast(float, key[j * V + v]);
      float gc = -INFINITY;
      if (gt != -INFINITY) {   // then s.g and z are finite, z >= gt
        const float d = gt - z;
        const float l1me = d > -0.6931472f ? logf(-expm1f(d)) : log1pf(-expf(d));   // -inf at d == 0
        const float u = (s.g - gt) + l1me;
        gc = s.g - fmaxf(u, 0.f) - log1pf(expf(-fabsf(u)));
      }
      key[j * V + v] = score_key(gc);   // never 0
    });
  }
  __syncthreads();

  const ExpandRows rows = {out_ids + b * k * (P + 1), out_g + b * k, out_phi + b * k, out_parent + b * k,
                           out_node + b * k};
  select_rounds<kExpMaxWaves>(key, N, k, nthr, [&](int r, uint32_t wk, int wi) {
    expand_write_row(rows, r, wk, wi, parents + b * kprev * P, V, P);
  });
  expand_nodes(rows, k, P, nd0, lvl);
  // the winner's phi: the value its Gt was formed from. A wave keeps the beam it formed last: on the first step every
  // row has the root for its parent, and one formation per wave serves them all.
  int last = -1;
  SampledBeam s = {};
  for (int r = wave; r < k; r += nwave) {
    const int v = (int)out_ids[(b * k + r) * (P + 1) + P];
    if (v < 0) continue;   // wave-uniform
    const int par = out_parent[b * k + r];
    const float* x = logits + (b * kprev + par) * V;
    if (par != last) {   // wave-uniform
      s = sampled_beam<BLOCKED, FILTERED>(par, lane, x, temperature, nd0, lvl, phi0, g0, V, flt);
      last = par;
    }
    if (lane == 0) out_phi[b * k + r] = sampled_child_phi(log_prob(x[v] / temperature - s.st.m, s.st), s);
  }
}

// ------------------------------------------------------------------------------------- expand, wide
// beam_expand_kernel's step without its dense key[kprev V] array, for up to kWideMax beams in and out: a user's
// candidates are enumerated, never stored. One workgroup of 16 waves per user.
//   1. a thread per beam: node -> child range (clamped as above; a range longer than V is cut at its first token >= V,
//      which a sorted range only ever loses skipped children to, and at V entries, so M <= kprev V fits an int), the
//      exclusive scan of the ranges' lengths: candidate e of the user's M is child lo[j] + e - off[j] of the beam j
//      with off[j] <= e < off[j + 1] (a binary search of off[] in LDS; every thread strides over e, whatever the
//      ranges' lengths). Then a wave per live beam, round robin: row_stats as beam_expand_kernel calls it, kept in LDS.
//   2. exact radix select of the k-th largest 64-bit key (score_key << 32 | ~(beam V + token): a strict total order
//      that is better()'s, so there are no ties to resolve): 8 bits per pass from the top through a 256-bin LDS
//      histogram; every pass enumerates the candidates again and wide_for_candidates forms each key anew from the
//      stored statistics — one function, the operations of beam_expand_kernel (log_prob(x / T - m) + plp: no
//      multiply-add pair to contract), for every pass and for the output. The passes stop at the first bin that holds
//      exactly the keys still needed (with fewer than k candidates: before the first).
//   3. one more enumeration collects the keys >= the cut with their child index — the winner's trie node, no search —
//      an LDS bitonic sort puts the <= kWideMax (key, node) pairs in output order, then the rows are written, the
//      parent prefixes gathered over k rows.
// Duplicate (beam, token) pairs (a bad table) make equal keys: more than k may pass the cut, the collection stops at
// kWideMax slots and k rows are written — which of the duplicates is unspecified, every index stays in bounds.
constexpr int kWideMax = 1024;
constexpr int kWideThreads = 1024;

struct WideBeams {   // LDS, per beam
  float m[kWideMax], sum[kWideMax], log_norm[kWideMax], plp[kWideMax];
  int lo[kWideMax], off[kWideMax + 1];   // first child; candidates before this beam (off[kprev] = M)
};

// the log-probability of token v on beam j (x the user's logits rows), the parent's added: beam_expand_kernel's
// operations, from the stored statistics
__device__ __forceinline__ float wide_lp(const WideBeams& s, const float* __restrict__ x, float temperature, int V,
                                         int j, int v) {
  const RowStats st = {s.m[j], s.sum[j], s.log_norm[j]};
  return log_prob(x[(int64_t)j * V + v] / temperature - st.m, st) + s.plp[j];
}

// f(key, c) for every candidate of the user that thread tid owns: c its level-(P + 1) node. BIASED: the key is formed
// from the biased score (ChildFilter::score), in every pass.
template <bool BLOCKED, bool FILTERED, bool BIASED = false, typename F>
__device__ __forceinline__ void wide_for_candidates(const WideBeams& s, const ChildFilter& flt,
                                                    const float* __restrict__ x, float temperature,
                                                    const int32_t* __restrict__ tok, int kprev, int V, F f) {
  const int M = s.off[kprev];
  for (int e = threadIdx.x; e < M; e += kWideThreads) {
    const int j = upper_bound(s.off, 0, kprev, e) - 1;
    const int c = s.lo[j] + (e - s.off[j]);
    const int v = tok[c];
    uint32_t sk;
    if constexpr (BIASED) {
      float add;
      if (!flt.candidate<BLOCKED, FILTERED, BIASED>(c, v, V, add)) continue;
      sk = score_key(flt.score<BIASED>(wide_lp(s, x, temperature, V, j, v), add));
    } else {
      if (!flt.candidate<BLOCKED, FILTERED>(c, v, V)) continue;
      sk = score_key(wide_lp(s, x, temperature, V, j, v));
    }
    f(((uint64_t)sk << 32) | (uint32_t)~(uint32_t)(j * V + v), c);
  }
}

// BIASED: the score written from the winner's key is out_score; out_lp is wide_lp of the winner's (beam, token), both
// known when the rows are written.
template <bool BLOCKED, bool FILTERED, bool BIASED = false>
__global__ void __launch_bounds__(kWideThreads) beam_expand_wide_kernel(
    const float* __restrict__ logits, float temperature, const int32_t* __restrict__ node, TrieLevel lvl,
    const int64_t* __restrict__ parents, const float* __restrict__ parent_lp, int kprev, int V, int P, int k,
    int64_t* __restrict__ out_ids, float* __restrict__ out_lp, int32_t* __restrict__ out_parent,
    int32_t* __restrict__ out_node, const int32_t* __restrict__ blocked, int n_blocked, ChildRows<BIASED> allowed) {
  __shared__ WideBeams s;
  __shared__ int hist[256];
  __shared__ uint64_t wkey[kWideMax];
  __shared__ int wnode[kWideMax];
  __shared__ int blk[BLOCKED ? kBlockedMax : 1];
  __shared__ int wsum[kWideThreads / 64];
  __shared__ int sel[3];   // the cut's bin (-1: none), the keys above it, the keys in it
  __shared__ int n_won;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t b = blockIdx.x;
  const float* x = logits + b * kprev * V;
  const ChildFilter flt = child_filter<FILTERED>(blk, n_blocked, allowed, b);

  // 1. child ranges and their scan
  int lo = 0, cnt = 0;
  if (tid < kprev) {
    int hi;
    if (lvl.children(node ? node[b * kprev + tid] : 0, lo, hi)) {
      if (hi - lo > V) hi = min(lower_bound(lvl.tok, lo, hi, V), lo + V);
      cnt = max(hi - lo, 0);
    }
    s.lo[tid] = lo;
    s.plp[tid] = parent_lp ? parent_lp[b * kprev + tid] : 0.0f;
  }
  if constexpr (BLOCKED) {
    for (int e = tid; e < n_blocked; e += kWideThreads) blk[e] = blocked[b * n_blocked + e];
  }
  int incl = cnt;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(incl, o, 64);
    if (lane >= o) incl += t;
  }
  if (lane == 63) wsum[wave] = incl;
  if (tid == 0) n_won = 0;
  __syncthreads();
  for (int w = 0; w < wave; ++w) incl += wsum[w];
  if (tid < kprev) s.off[tid] = incl - cnt;
  if (tid == kWideThreads - 1) s.off[kprev] = incl;   // threads past kprev add nothing: the total
  __syncthreads();
  for (int j = wave; j < kprev; j += kWideThreads / 64) {
    if (s.off[j + 1] == s.off[j]) continue;   // a dead beam or an empty range (wave-uniform)
    const float* xr = x + (int64_t)j * V;
    const RowStats st = row_stats<0>(
        V, lane, [&](int, int v) { return xr[v] / temperature; },
        [&](int, int v, float m) { return xr[v] / temperature - m; });
    if (lane == 0) { s.m[j] = st.m; s.sum[j] = st.sum; s.log_norm[j] = st.log_norm; }
  }

  // 2. the cut: the k-th largest key, or 0 with fewer than k candidates
  uint64_t cut = 0;
  int need = k;
#pragma unroll 1
  for (int shift = 56; shift >= 0; shift -= 8) {
    if (tid < 256) hist[tid] = 0;
    __syncthreads();   // also: the statistics are written
    const uint64_t above = shift == 56 ? 0 : ~0ull << (shift + 8);   // the digits already fixed
    wide_for_candidates<BLOCKED, FILTERED, BIASED>(s, flt, x, temperature, lvl.tok, kprev, V, [&](uint64_t key, int) {
      if ((key & above) == cut) atomicAdd(&hist[(int)(key >> shift) & 255], 1);
    });
    __syncthreads();
    if (wave == 0) {   // lane l: bins 255 - 4 l down to 252 - 4 l; the first bin, from the top, that reaches `need`
      int h[4], sum = 0;
#pragma unroll
      for (int t = 0; t < 4; ++t) sum += h[t] = hist[255 - 4 * lane - t];
      int run = sum;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(run, o, 64);
        if (lane >= o) run += t;
      }
      const uint64_t reach = __ballot(run >= need);
      if (!reach) {
        if (lane == 0) sel[0] = -1;
      } else if (lane == __ffsll((unsigned long long)reach) - 1) {
        int acc = run - sum, d = -1, in_d = 0;   // this lane's bins reach `need`
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          if (d < 0 && acc + h[t] >= need) { d = 255 - 4 * lane - t; in_d = h[t]; }
          if (d < 0) acc += h[t];
        }
        sel[0] = d;
        sel[1] = acc;
        sel[2] = in_d;
      }
    }
    __syncthreads();
    if (sel[0] < 0) break;   // fewer than k candidates (first pass only): all of them
    cut |= (uint64_t)sel[0] << shift;
    need -= sel[1];
    if (sel[2] == need) break;   // the bin holds exactly the keys still needed
  }

  // 3. collect, sort, write
  wide_for_candidates<BLOCKED, FILTERED, BIASED>(s, flt, x, temperature, lvl.tok, kprev, V, [&](uint64_t key, int c) {
    if (key >= cut) {
      const int at = atomicAdd(&n_won, 1);
      if (at < kWideMax) { wkey[at] = key; wnode[at] = c; }
    }
  });
  __syncthreads();
  const int n = min(n_won, kWideMax);
  int n2 = 1;
  while (n2 < n) n2 <<= 1;
  if (tid >= n && tid < n2) wkey[tid] = 0;   // below every key
  __syncthreads();
  for (int kk = 2; kk <= n2; kk <<= 1) {
    for (int jj = kk >> 1; jj > 0; jj >>= 1) {
      const int o = tid ^ jj;
      if (tid < n2 && o > tid) {
        const uint64_t a = wkey[tid], c = wkey[o];
        if ((a < c) == ((tid & kk) == 0)) {   // descending
          const int na = wnode[tid];
          wkey[tid] = c; wkey[o] = a;
          wnode[tid] = wnode[o]; wnode[o] = na;
        }
      }
      __syncthreads();
    }
  }
  const int live = min(n, k);
  if (tid < k) {
    const bool dead = tid >= live;
    const uint64_t key = dead ? 0 : wkey[tid];
    if constexpr (BIASED) {
      const int at = (int)~(uint32_t)key, par = at / V;
      allowed.out_score[b * k + tid] = dead ? -INFINITY : key_score((uint32_t)(key >> 32));
      out_lp[b * k + tid] = dead ? -INFINITY : wide_lp(s, x, temperature, V, par, at - par * V);
    } else {
      out_lp[b * k + tid] = dead ? -INFINITY : key_score((uint32_t)(key >> 32));
    }
    out_parent[b * k + tid] = dead ? 0 : (int)(~(uint32_t)key) / V;
    out_node[b * k + tid] = dead ? -1 : wnode[tid];
  }
  for (int e = tid; e < k * (P + 1); e += kWideThreads) {
    const int r = e / (P + 1), t = e - r * (P + 1);
    int64_t id = -1;
    if (r < live) {
      const int at = (int)~(uint32_t)wkey[r], par = at / V;
      id = t < P ? parents[(b * kprev + par) * P + t] : at - par * V;
    }
    out_ids[b * k * (P + 1) + e] = id;
  }
}

// ------------------------------------------------------------------------------------- score paths
// Teacher-forced scoring: the log-probability of the token every one of a user's C candidates names at this step, in
// beam_expand_kernel's arithmetic (the same functions: row_stats, log_prob), so a candidate's score is bitwise what
// rq_beam_expand gives the same (row, token, parent score). One workgroup per user.
//   G == 1 (step 0): the user's candidates share the BOS row. Every wave forms the row's statistics itself (the same
//          function gives the same bits, so no barrier), then the threads stride over the candidates.
//   G == C (later steps): a wave per candidate row, round robin. The row is read from memory once, into J registers
//          per lane (J = 4 / 16 / 64 by V, picked on the host); only the named class is fetched again (one dword).
// A padding candidate (present[b][c] == 0) gets -inf, its row is never read and its token is never used; a present
// candidate whose token is outside [0, V) gets -inf without touching its row (and stays -inf: -inf + prev_lp).
// out_rank: the scores' keys stay in LDS (0 for padding: below every float's key) and rank[c] counts the candidates
// that are better(...) than c — a permutation of 0..C-1, ties to the lower index, real -inf above padding.
// Waves per workgroup in the G == C form: 16 (as beam_expand_kernel's latency-bound phase) for J <= 16; 8 for J = 64,
// whose 64 row registers per lane do not fit the 128 VGPRs a 16-wave workgroup leaves a lane.
template <int J>
constexpr int kScoreWaves = J <= 16 ? 16 : 8;

// row_stats of one row that every lane holds in registers, z[j] = x[lane + 64 j] / T: read from memory once
template <int J>
__device__ __forceinline__ RowStats score_row_stats(const float* __restrict__ x, int V, float temperature, int lane) {
  float z[J];
  return row_stats<J>(
      V, lane, [&](int j, int v) { return z[j] = x[v] / temperature; }, [&](int j, int, float m) { return z[j] - m; });
}

template <int J>
__global__ void __launch_bounds__(64 * kScoreWaves<J>) score_paths_kernel(
    const float* __restrict__ logits, float temperature, const int64_t* __restrict__ tokens, int64_t tok_sb,
    int64_t tok_sc, const bool* __restrict__ present, const float* __restrict__ prev_lp, int C, int V, int G,
    float* __restrict__ out_lp, int32_t* __restrict__ out_rank) {
  __shared__ uint32_t key[kRankMaxK];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nthr = blockDim.x, nwave = nthr >> 6;
  const int64_t b = blockIdx.x;
  const int64_t* tk = tokens + b * tok_sb;
  const int64_t bc = b * C;

  if (G == 1) {
    const float* x = logits + b * V;
    const RowStats st = score_row_stats<J>(x, V, temperature, lane);
    for (int c = tid; c < C; c += nthr) {
      const bool pr = !present || present[bc + c];
      float out = -INFINITY;
      if (pr) {
        const int64_t t = tk[c * tok_sc];
        if (t >= 0 && t < V) out = log_prob(x[t] / temperature - st.m, st) + (prev_lp ? prev_lp[bc + c] : 0.0f);
      }
      out_lp[bc + c] = out;
      key[c] = pr ? score_key(out) : 0;
    }
  } else {
    for (int c = wave; c < C; c += nwave) {   // everything below is wave-uniform
      const bool pr = !present || present[bc + c];
      float out = -INFINITY;
      if (pr) {
        const int64_t t = tk[c * tok_sc];
        if (t >= 0 && t < V) {
          const float* x = logits + (bc + c) * V;
          const RowStats st = score_row_stats<J>(x, V, temperature, lane);
          out = log_prob(x[t] / temperature - st.m, st) + (prev_lp ? prev_lp[bc + c] : 0.0f);
        }
      }
      if (lane == 0) {
        out_lp[bc + c] = out;
        key[c] = pr ? score_key(out) : 0;
      }
    }
  }
  if (!out_rank) return;   // workgroup-uniform
  __syncthreads();
  for (int c = tid; c < C; c += nthr) {
    const uint32_t kc = key[c];
    int cnt = 0;
    for (int u = 0; u < C; ++u) cnt += better(key[u], u, kc, c);   // every lane reads key[u]: an LDS broadcast
    out_rank[bc + c] = cnt;
  }
}

template <int J>
static void launch_score_paths(const float* logits, float temperature, const int64_t* tokens, int64_t tok_sb,
                               int64_t tok_sc, const bool* present, const float* prev_lp, int64_t B, int C, int V,
                               int G, float* out_lp, int32_t* out_rank, hipStream_t stream) {
  const int waves = (G == 1 || C <= 4) ? 4 : kScoreWaves<J>;
  hipLaunchKernelGGL(score_paths_kernel<J>, dim3((unsigned)B), dim3(64 * waves), 0, stream, logits, temperature,
                     tokens, tok_sb, tok_sc, present, prev_lp, C, V, G, out_lp, out_rank);
}

// ------------------------------------------------------------------------------------- self-attention
// The step buffers by value in the kernel arguments (no device-side pointer table): K / V column views of step
// s's packed qkv output, its row stride and row count.
struct BeamSteps {
  const float* k[RQ_BEAM_MAX_T];
  const float* v[RQ_BEAM_MAX_T];
  int64_t stride[RQ_BEAM_MAX_T];
  int64_t rows[RQ_BEAM_MAX_T];
};

// LPU = hd / 4 lanes per (row, head) unit, 256 / LPU units per workgroup. A lane holds 4 consecutive head
// columns: one float4 of q, and per step one float4 of the ancestor's key and value row; the dot product is a
// butterfly sum inside the unit. Bandwidth-bound: 4 R H hd (2 (t + 1) + 2) bytes, no LDS. Scores, max and the
// sum over s = 0..t (ascending) in fp32; at t == 0 the weight is exp(0) / 1, so out == v bitwise.
// anc entries are not validated (the caller's contract: in [0, rows[s])); they are clamped to the step's
// buffer, so a bad entry gives an unspecified result but never a read outside it.
template <int LPU>
__global__ void __launch_bounds__(256) beam_self_attn_kernel(const float* __restrict__ q, int64_t sq, BeamSteps st,
                                                             const int32_t* __restrict__ anc, int64_t units, int H,
                                                             int t, float scale, float* __restrict__ out,
                                                             int64_t so) {
  const int64_t u_raw = ((int64_t)blockIdx.x * 256 + threadIdx.x) / LPU;
  const bool live = u_raw < units;
  const int64_t u = live ? u_raw : units - 1;   // idle units repeat the last one (whole-wave shuffles), write nothing
  const int64_t r = u / H;
  const int col = (int)(u % H) * (LPU * 4) + (int)(threadIdx.x % LPU) * 4;
  const float4 qv = *reinterpret_cast<const float4*>(q + r * sq + col);
  float sc[RQ_BEAM_MAX_T];
  float4 vv[RQ_BEAM_MAX_T];
  float m = -INFINITY;
#pragma unroll
  for (int s = 0; s < RQ_BEAM_MAX_T; ++s) {
    if (s <= t) {
      int64_t row = r;
      if (s < t) row = min(max((int64_t)anc[r * t + s], (int64_t)0), st.rows[s] - 1);
      const int64_t off = row * st.stride[s] + col;
      const float4 kv = *reinterpret_cast<const float4*>(st.k[s] + off);
      vv[s] = *reinterpret_cast<const float4*>(st.v[s] + off);
      const float d = group_sum<LPU>(qv.x * kv.x + qv.y * kv.y + qv.z * kv.z + qv.w * kv.w);
      sc[s] = d * scale;
      m = fmaxf(m, sc[s]);
    }
  }
  // s = 0 always exists; later terms are added in step order
  float l = expf(sc[0] - m);
  float4 acc = make_float4(l * vv[0].x, l * vv[0].y, l * vv[0].z, l * vv[0].w);
#pragma unroll
  for (int s = 1; s < RQ_BEAM_MAX_T; ++s) {
    if (s <= t) {
      const float p = expf(sc[s] - m);
      l += p;
      acc.x += p * vv[s].x;
      acc.y += p * vv[s].y;
      acc.z += p * vv[s].z;
      acc.w += p * vv[s].w;
    }
  }
  if (live) *reinterpret_cast<float4*>(out + r * so + col) = make_float4(acc.x / l, acc.y / l, acc.z / l, acc.w / l);
}

template <int LPU>
static void launch_beam_self_attn(const float* q, int64_t sq, const BeamSteps& st, const int32_t* anc, int64_t units,
                                  int H, int t, float scale, float* out, int64_t so, hipStream_t stream) {
  const int64_t blocks = (units * LPU + 255) / 256;
  hipLaunchKernelGGL(beam_self_attn_kernel<LPU>, dim3((unsigned)blocks), dim3(256), 0, stream, q, sq, st, anc, units,
                     H, t, scale, out, so);
}

// ------------------------------------------------------------------------------------- hits
struct HitKs {
  int v[kHitsMaxKs];
};

// Lane i < D carries column i's two first-match ranks of the current row and its counters; beams are
// visited 64 at a time, one per lane: bit i of a lane's `pos` says its beam equals the target in column i,
// `slice` has bit i where columns 0..i all match (the trailing ones of pos).
__global__ void __launch_bounds__(256) topk_hits_kernel(const int64_t* __restrict__ actual,
                                                        const int64_t* __restrict__ topk, int64_t B, int k, int D,
                                                        HitKs ks, int n_ks,
                                                        unsigned long long* __restrict__ counts) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  int c_slice[kHitsMaxKs], c_pos[kHitsMaxKs];
#pragma unroll
  for (int j = 0; j < kHitsMaxKs; ++j) c_slice[j] = c_pos[j] = 0;
  for (int64_t row = wave; row < B; row += n_waves) {
    const int64_t* a = actual + row * D;
    int r_slice = kNoRank, r_pos = kNoRank;
    for (int r0 = 0; r0 < k; r0 += 64) {
      const int r = r0 + lane;
      uint64_t pos = 0;
      if (r < k) {
        const int64_t* t = topk + (row * k + r) * D;
        for (int i = 0; i < D; ++i) pos |= (uint64_t)(t[i] == a[i]) << i;
      }
      const uint64_t slice = ~pos & (pos + 1) ? (~pos & (pos + 1)) - 1 : ~0ull;
      int missing = 0;
      for (int i = 0; i < D; ++i) {
        const uint64_t bp = __ballot((pos >> i) & 1);
        const uint64_t bs = __ballot((slice >> i) & 1);
        if (lane == i) {
          if (r_pos == kNoRank && bp) r_pos = r0 + __ffsll((unsigned long long)bp) - 1;
          if (r_slice == kNoRank && bs) r_slice = r0 + __ffsll((unsigned long long)bs) - 1;
          missing = r_pos == kNoRank || r_slice == kNoRank;
        }
      }
      if (!__any(missing)) break;
    }
#pragma unroll
    for (int j = 0; j < kHitsMaxKs; ++j) {
      if (j < n_ks) {
        c_slice[j] += r_slice < ks.v[j];
        c_pos[j] += r_pos < ks.v[j];
      }
    }
  }
  if (lane < D) {
#pragma unroll
    for (int j = 0; j < kHitsMaxKs; ++j) {
      if (j < n_ks) {
        if (c_slice[j]) atomicAdd(&counts[(size_t)lane * n_ks + j], (unsigned long long)c_slice[j]);
        if (c_pos[j]) atomicAdd(&counts[((size_t)D + lane) * n_ks + j], (unsigned long long)c_pos[j]);
      }
    }
  }
}

// ------------------------------------------------------------------------------------- rank histogram
// One wave per row (grid-stride): beams are visited 64 at a time, one per lane; the first 64-block with a beam equal
// to the target in all D columns gives the rank. Lane 0 counts into the workgroup's LDS histogram, which is flushed
// with one global atomic per non-empty bin: integer counts, so the result does not depend on the order.
__global__ void __launch_bounds__(256) rank_hist_kernel(const int64_t* __restrict__ actual,
                                                        const int64_t* __restrict__ topk, int64_t B, int k, int D,
                                                        unsigned long long* __restrict__ hist) {
  __shared__ int h[kRankMaxK + 1];
  const int lane = threadIdx.x & 63;
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int i = threadIdx.x; i <= k; i += blockDim.x) h[i] = 0;
  __syncthreads();
  for (int64_t row = wave; row < B; row += n_waves) {
    const int64_t* a = actual + row * D;
    if (a[0] < 0) continue;   // no target (wave-uniform)
    int rank = k;
    for (int r0 = 0; r0 < k; r0 += 64) {
      const int r = r0 + lane;
      bool eq = r < k;
      if (eq) {
        const int64_t* t = topk + (row * k + r) * D;
        for (int i = 0; i < D; ++i) eq = eq && t[i] == a[i];
      }
      const uint64_t hit = __ballot(eq);
      if (hit) {
        rank = r0 + __ffsll((unsigned long long)hit) - 1;
        break;
      }
    }
    if (lane == 0) atomicAdd(&h[rank], 1);
  }
  __syncthreads();
  for (int i = threadIdx.x; i <= k; i += blockDim.x)
    if (h[i]) atomicAdd(&hist[i], (unsigned long long)h[i]);
}

// ------------------------------------------------------------------------------------- blocked trie nodes
// The per-level tables by value in the kernel arguments (no device-side pointer table): level q = 1..D at [q - 1].
struct TrieLevels {
  const int32_t* anc[RQ_BEAM_MAX_T];   // (n_leaves): each leaf's level-q ancestor
  const int32_t* cnt[RQ_BEAM_MAX_T];   // (n_nodes[q - 1]): each level-q node's number of leaves
  int n_nodes[RQ_BEAM_MAX_T];
};

constexpr int kBlkThreads = 256;
constexpr int kBlkNone = 0x7fffffff;

// ascending bitonic sort of s[0, n), n a power of two <= kBlockedMax; starts and ends with a barrier
__device__ __forceinline__ void lds_sort(int* s, int n) {
  __syncthreads();
  for (int k = 2; k <= n; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = threadIdx.x; i < n; i += kBlkThreads) {
        const int o = i ^ j;
        if (o > i) {
          const int a = s[i], c = s[o];
          if ((a > c) == ((i & k) == 0)) { s[i] = c; s[o] = a; }
        }
      }
      __syncthreads();
    }
  }
}

// One workgroup per user. The user's listed items become leaves (an entry outside [0, n_items) is padding), sorted
// and made distinct in LDS: leaf[0, n) ascending. A level's nodes are in key order, so the leaves' level-q ancestors
// are non-decreasing: a node is blocked iff its run in that sequence is as long as its leaf count (all of its leaves
// are listed). The run heads that qualify are sorted once more, which moves them to the front of the output row in
// ascending order with the INT32_MAX padding behind. Table values are never trusted for addressing: a leaf outside
// [0, n_leaves) is padding, an ancestor outside [0, n_nodes) is never blocked.
__global__ void __launch_bounds__(kBlkThreads) trie_blocked_kernel(const int64_t* __restrict__ items, int H, int Hp,
                                                                  const int32_t* __restrict__ item_leaf,
                                                                  int64_t n_items, int n_leaves, TrieLevels lv, int D,
                                                                  int64_t B, int32_t* __restrict__ out) {
  __shared__ int leaf[kBlockedMax];
  __shared__ int anc[kBlockedMax];
  __shared__ int res[kBlockedMax];
  const int tid = threadIdx.x;
  const int64_t b = blockIdx.x;
  for (int i = tid; i < Hp; i += kBlkThreads) {
    int lf = kBlkNone;
    if (i < H) {
      const int64_t it = items[b * H + i];
      if (it >= 0 && it < n_items) {
        lf = item_leaf[it];
        if (lf < 0 || lf >= n_leaves) lf = kBlkNone;
      }
    }
    leaf[i] = lf;
  }
  lds_sort(leaf, Hp);
  for (int i = tid; i < Hp; i += kBlkThreads) res[i] = (i > 0 && leaf[i] == leaf[i - 1]) ? kBlkNone : leaf[i];
  __syncthreads();
  for (int i = tid; i < Hp; i += kBlkThreads) leaf[i] = res[i];
  lds_sort(leaf, Hp);
  // n = the number of distinct leaves: the first padding entry of the ascending row
  const int n = lower_bound(leaf, 0, Hp, kBlkNone);
#pragma unroll 1
  for (int q = 0; q < D; ++q) {
    const int32_t* aq = lv.anc[q];
    const int32_t* cq = lv.cnt[q];
    const int nq = lv.n_nodes[q];
    for (int i = tid; i < Hp; i += kBlkThreads) anc[i] = i < n ? aq[leaf[i]] : kBlkNone;
    __syncthreads();
    for (int i = tid; i < Hp; i += kBlkThreads) {
      int r = kBlkNone;
      const int a = anc[i];
      if (i < n && a >= 0 && a < nq && (i == 0 || anc[i - 1] != a)) {
        if (upper_bound(anc, i + 1, n, a) - i == cq[a]) r = a;   // the end of a's run
      }
      res[i] = r;
    }
    lds_sort(res, Hp);
    int32_t* o = out + ((int64_t)q * B + b) * H;
    for (int i = tid; i < H; i += kBlkThreads) o[i] = res[i];
    __syncthreads();   // anc / res are rewritten by the next level
  }
}

// ------------------------------------------------------------------------------------- allowed trie nodes
// Catalogue filters: mask (G, N) bool says which corpus items group g may be shown. Per group, level q = 1..D gets a
// bitmap over its nodes (bit c & 31 of word c >> 5: node c has an allowed item below it) and every leaf the lowest
// allowed item whose row it is. Both are reductions that do not depend on the order (bit OR, index MIN), so the result
// is the same in every run. The outputs arrive zeroed.
//   trie_allowed_kernel  a thread per 4 consecutive mask bytes (one dword load where the mask is 4-byte aligned), grid
//                        stride. For an allowed item i of group g with leaf l: atomicMax of ~i into lowest[g][l] (the
//                        largest ~i is the lowest i, and the zero it starts from is ~(-1): "none"), and for every level
//                        the bit of l's ancestor — tested with a plain load first, the atomic OR only where it is still
//                        clear: the upper levels have a handful of words per group, which every allowed item below
//                        them would otherwise hit.
//   trie_allowed_finish_kernel  lowest[g][l] = ~lowest[g][l] in place: the item, or -1.
// Table values are never trusted for addressing: a leaf outside [0, n_leaves) or an ancestor outside [0, n_nodes) is
// skipped.
struct AllowedLevels {
  const int32_t* anc[RQ_BEAM_MAX_T];   // (n_leaves): each leaf's level-q ancestor
  int32_t* bits[RQ_BEAM_MAX_T];        // (G, n_words[q - 1]), zeroed
  int n_nodes[RQ_BEAM_MAX_T];
  int n_words[RQ_BEAM_MAX_T];          // ceil(n_nodes / 32)
};

constexpr int kAllowThreads = 256;
constexpr int kAllowMaxBlocks = 2048;

__global__ void __launch_bounds__(kAllowThreads) trie_allowed_kernel(const uint8_t* __restrict__ mask, int64_t G,
                                                                    int64_t n_items,
                                                                    const int32_t* __restrict__ item_leaf,
                                                                    int n_leaves, AllowedLevels lv, int D,
                                                                    unsigned long long* __restrict__ lowest) {
  const int64_t total = G * n_items;
  const bool aligned = (reinterpret_cast<uintptr_t>(mask) & 3) == 0;
  const int64_t stride = (int64_t)gridDim.x * kAllowThreads * 4;
  for (int64_t e0 = ((int64_t)blockIdx.x * kAllowThreads + threadIdx.x) * 4; e0 < total; e0 += stride) {
    uint32_t m = 0;   // byte t: mask[e0 + t]
    if (aligned && e0 + 4 <= total) {
      m = *reinterpret_cast<const uint32_t*>(mask + e0);
    } else {
      for (int t = 0; t < 4; ++t)
        if (e0 + t < total) m |= (uint32_t)mask[e0 + t] << (8 * t);
    }
    if (m == 0) continue;
    for (int t = 0; t < 4; ++t) {
      if (((m >> (8 * t)) & 0xffu) == 0) continue;
      const int64_t g = (e0 + t) / n_items, item = (e0 + t) - g * n_items;
      const int leaf = item_leaf[item];
      if (leaf < 0 || leaf >= n_leaves) continue;
      unsigned long long* lw = lowest + g * n_leaves + leaf;
      const unsigned long long enc = ~(unsigned long long)item;
      if (__atomic_load_n(lw, __ATOMIC_RELAXED) < enc) atomicMax(lw, enc);
#pragma unroll 1
      for (int q = 0; q < D; ++q) {
        const int a = lv.anc[q][leaf];
        if (a < 0 || a >= lv.n_nodes[q]) continue;
        int32_t* w = lv.bits[q] + g * lv.n_words[q] + (a >> 5);
        const int32_t bit = (int32_t)(1u << (a & 31));
        if (!(__atomic_load_n(w, __ATOMIC_RELAXED) & bit)) atomicOr(w, bit);
      }
    }
  }
}

__global__ void __launch_bounds__(kAllowThreads) trie_allowed_finish_kernel(unsigned long long* __restrict__ lowest,
                                                                           int64_t n) {
  const int64_t stride = (int64_t)gridDim.x * kAllowThreads;
  for (int64_t i = (int64_t)blockIdx.x * kAllowThreads + threadIdx.x; i < n; i += stride) lowest[i] = ~lowest[i];
}

// ------------------------------------------------------------------------------------- bias bounds of trie nodes
// Per-item score bias: bias (G, N) fp32 says what group g adds to item i's score. Per group, level q = 1..D gets every
// node's bound — the largest cleaned bias (clean_bias) of an item below it, -inf with none: what a completion of that
// prefix can still gain — and every leaf the item that attains its bound, the lowest index among equals (-1 at -inf).
// Both are integer maxima, which do not depend on the order, so two runs give the same bits; no float atomic is used.
// The outputs arrive zeroed.
//   trie_bias_kernel  a thread per (group, item), grid stride. An item whose cleaned bias is -inf is skipped: it can
//                     raise no bound. Else, with k = score_key(bias) (monotone, never 0) and leaf l: atomicMax of
//                     (k << 32 | ~i) into best[g][l] (the largest key, then the lowest i), and atomicMax of k into the
//                     bound of l's ancestor at every level — each tested with a plain load first, the atomic only
//                     where it would still raise the value (the upper levels have a handful of nodes per group).
//   trie_bias_finish_kernel  in place: a bound's key back to its float (0, never raised: -inf), best[g][l] to the
//                     item (0: -1).
// Table values are never trusted for addressing: a leaf outside [0, n_leaves) or an ancestor outside [0, n_nodes) is
// skipped.
struct BiasLevels {
  const int32_t* anc[RQ_BEAM_MAX_T];   // (n_leaves): each leaf's level-q ancestor
  uint32_t* upper[RQ_BEAM_MAX_T];      // (G, n_nodes[q - 1]), zeroed: keys while reducing, floats after the finish
  int n_nodes[RQ_BEAM_MAX_T];
};

__global__ void __launch_bounds__(kAllowThreads) trie_bias_kernel(const float* __restrict__ bias, int64_t G,
                                                                 int64_t n_items,
                                                                 const int32_t* __restrict__ item_leaf, int n_leaves,
                                                                 BiasLevels lv, int D,
                                                                 unsigned long long* __restrict__ best) {
  const int64_t total = G * n_items;
  const int64_t stride = (int64_t)gridDim.x * kAllowThreads;
  for (int64_t e = (int64_t)blockIdx.x * kAllowThreads + threadIdx.x; e < total; e += stride) {
    const float u = clean_bias(bias[e]);
    if (u == -INFINITY) continue;
    const uint32_t key = score_key(u);
    const int64_t g = e / n_items, item = e - g * n_items;
    const int leaf = item_leaf[item];
    if (leaf < 0 || leaf >= n_leaves) continue;
    unsigned long long* bw = best + g * n_leaves + leaf;
    const unsigned long long enc = ((unsigned long long)key << 32) | (uint32_t)~(uint32_t)item;
    if (__atomic_load_n(bw, __ATOMIC_RELAXED) < enc) atomicMax(bw, enc);
#pragma unroll 1
    for (int q = 0; q < D; ++q) {
      const int a = lv.anc[q][leaf];
      if (a < 0 || a >= lv.n_nodes[q]) continue;
      uint32_t* w = lv.upper[q] + g * lv.n_nodes[q] + a;
      if (__atomic_load_n(w, __ATOMIC_RELAXED) < key) atomicMax(w, key);
    }
  }
}

__global__ void __launch_bounds__(kAllowThreads) trie_bias_finish_kernel(BiasLevels lv, int D, int64_t G,
                                                                        unsigned long long* __restrict__ best,
                                                                        int64_t n_best) {
  const int64_t stride = (int64_t)gridDim.x * kAllowThreads;
  const int64_t first = (int64_t)blockIdx.x * kAllowThreads + threadIdx.x;
#pragma unroll 1
  for (int q = 0; q < D; ++q) {
    uint32_t* up = lv.upper[q];
    const int64_t n = G * lv.n_nodes[q];
    for (int64_t i = first; i < n; i += stride) {
      const uint32_t key = up[i];
      up[i] = __builtin_bit_cast(uint32_t, key == 0 ? -INFINITY : key_score(key));
    }
  }
  for (int64_t i = first; i < n_best; i += stride) {
    const unsigned long long v = best[i];
    best[i] = v == 0 ? ~0ull : (unsigned long long)(uint32_t)~(uint32_t)v;
  }
}

// Host side of the expand kernels: f(BLOCKED, FILTERED, BIASED), the three as std::bool_constant values — the one
// instantiation the tables given ask for. BiasArgs: BIASED, never FILTERED; AllowedBits: FILTERED iff it has a group.
template <typename Rows, typename F>
static void with_tables(bool blocked, const Rows& rows, F f) {
  constexpr bool kBia = std::is_same_v<Rows, BiasArgs>;
  auto blk = [&](auto flt) {
    if (blocked) f(std::true_type{}, flt, std::bool_constant<kBia>{});
    else f(std::false_type{}, flt, std::bool_constant<kBia>{});
  };
  if constexpr (kBia) blk(std::false_type{});
  else if (rows.group != nullptr) blk(std::true_type{});
  else blk(std::false_type{});
}

// An int64 size of the C ABI as the int of a kernel argument struct; where it does not fit, -1, which every check refuses
static int arg_int(int64_t v) { return v < 0 || v > 0x7fffffff ? -1 : (int)v; }

// The argument checks of the three expand entry points, in one order; fn is the entry point's name for the message.
// beams_ok / beam_names: the P == 0 rule over the entry point's own beam arrays; own_ptrs: its logits and outputs; ab:
// its catalogue bitmap, NULL where it takes none. After a 0 the caller still returns at once when B == 0 (nothing is
// dereferenced, NULL is fine then).
enum class ExpandForm { kDense, kWide, kSampled };
static int beam_expand_check(const char* fn, ExpandForm form, float temperature, int64_t n_nodes, const int32_t* tok,
                             int64_t n_children, bool beams_ok, const char* beam_names, int64_t B, int64_t kprev,
                             int64_t V, int64_t P, int64_t k, bool own_ptrs, const int32_t* blocked, int64_t n_blocked,
                             const AllowedBits* ab) {
  const bool filtered = ab && ab->group;
  RQ_CHECK_ARG(B >= 0 && kprev >= 1 && V >= 1 && P >= 0 && P < 64, "%s: bad shape", fn);
  if (form == ExpandForm::kWide) {
    RQ_CHECK_ARG(V <= kBeamMaxV && kprev <= kWideMax && k >= 1 && k <= kWideMax,
                 "%s: need V <= %d, kprev <= %d and 1 <= k <= %d (kprev=%lld, V=%lld, k=%lld)", fn, kBeamMaxV,
                 kWideMax, kWideMax, (long long)kprev, (long long)V, (long long)k);
  } else {
    RQ_CHECK_ARG(V <= kBeamMaxV && kprev <= kBeamMaxN && kprev * V <= kBeamMaxN,
                 "%s: need V <= %d and kprev * V <= %d (kprev=%lld, V=%lld)%s", fn, kBeamMaxV, kBeamMaxN,
                 (long long)kprev, (long long)V,
                 form == ExpandForm::kSampled
                     ? "; the wide form (more than 32 beams at V = 256) is not built for the sampled step"
                     : "");
    RQ_CHECK_ARG(k >= 1 && k <= kBeamMaxN, "%s: need 1 <= k <= %d (k=%lld)", fn, kBeamMaxN, (long long)k);
  }
  RQ_CHECK_ARG(temperature > 0.f && temperature <= 3.0e38f, "%s: temperature must be positive", fn);
  RQ_CHECK_ARG(n_nodes >= 0 && n_nodes < 0x7fffffff && n_children >= 0 && n_children <= 0x7fffffff,
               "%s: bad trie level (n_nodes=%lld, n_children=%lld)", fn, (long long)n_nodes, (long long)n_children);
  RQ_CHECK_ARG(beams_ok, "%s: %s are all NULL when P == 0, all given otherwise", fn, beam_names);
  RQ_CHECK_ARG(n_blocked >= 0 && n_blocked <= kBlockedMax, "%s: need 0 <= n_blocked <= %d (n_blocked=%lld)", fn,
               kBlockedMax, (long long)n_blocked);
  RQ_CHECK_ARG(!filtered || (ab->n_words >= 0 && ab->n_words <= 0x7fffffff / 32 && ab->G >= 0),
               "%s: bad bitmap (n_words=%d, G=%d)", fn, filtered ? ab->n_words : 0, filtered ? ab->G : 0);
  if (B == 0) return 0;
  RQ_CHECK_ARG(B <= 0x7fffffff, "%s: too many batch elements", fn);
  RQ_CHECK_ARG(own_ptrs && (tok || n_children == 0) && (blocked || n_blocked == 0) &&
                   (!filtered || ab->bits || (int64_t)ab->n_words * ab->G == 0),
               "%s: null pointer", fn);
  return 0;
}

static size_t beam_expand_lds(int64_t kprev, int64_t V, int64_t n_blocked, bool biased) {   // expand_prologue's layout
  return (size_t)((kprev * V + 3) / 4 * 4 + 2 * kExpMaxWaves) * sizeof(uint32_t) +
         (size_t)n_blocked * sizeof(int32_t) + (biased ? (size_t)kprev * 3 * sizeof(float) : 0);
}

// The four deterministic entry points; rows: the form's own kernel argument, sizes through arg_int, checked here.
template <typename Rows>
static int beam_expand_launch(const char* fn, bool wide, const float* logits, float temperature, const int32_t* node,
                              const int32_t* child_off, int64_t n_nodes, const int32_t* tok, int64_t n_children,
                              const int64_t* parents, const float* parent_lp, int64_t B, int64_t kprev, int64_t V,
                              int64_t P, int64_t k, int64_t* out_ids, float* out_lp, int32_t* out_parent,
                              int32_t* out_node, const int32_t* blocked, int64_t n_blocked, const Rows& rows,
                              void* stream) {
  bool own_ptrs = logits && child_off && out_ids && out_lp && out_parent && out_node;
  const AllowedBits* ab = nullptr;
  if constexpr (std::is_same_v<Rows, BiasArgs>) {
    RQ_CHECK_ARG(rows.n_bias >= 0 && rows.G >= 0 && rows.n_bias == n_children,
                 "%s: need G >= 0 and n_bias == n_children (n_bias=%d, n_children=%lld, G=%d)", fn, rows.n_bias,
                 (long long)n_children, rows.G);
    RQ_CHECK_ARG(rows.rows || rows.G == 0 || rows.n_bias == 0, "%s: null bias", fn);
    RQ_CHECK_ARG(wide || kprev <= kWideMax, "%s: the biased step takes kprev <= %d (kprev=%lld)", fn,
                 kWideMax, (long long)kprev);
    own_ptrs = own_ptrs && rows.out_score;
  } else {
    ab = &rows;
  }
  const int rc = beam_expand_check(
      fn, wide ? ExpandForm::kWide : ExpandForm::kDense, temperature, n_nodes, tok, n_children,
      (P == 0) ? (!node && !parents && !parent_lp) : (node && parents && parent_lp), "node, parents and parent_lp", B,
      kprev, V, P, k, own_ptrs, blocked, n_blocked, ab);
  if (rc != 0 || B == 0) return rc;
  const TrieLevel lvl = {child_off, (int)n_nodes, tok, (int)n_children};
  if (n_blocked == 0) blocked = nullptr;
  with_tables(n_blocked > 0, rows, [&](auto blk, auto flt, auto bia) {
    constexpr bool kBlk = decltype(blk)::value, kFlt = decltype(flt)::value, kBia = decltype(bia)::value;
    auto launch = [&](auto kernel, int threads, size_t lds) {
      hipLaunchKernelGGL(kernel, dim3((unsigned)B), dim3(threads), lds, (hipStream_t)stream, logits, temperature, node,
                         lvl, parents, parent_lp, (int)kprev, (int)V, (int)P, (int)k, out_ids, out_lp, out_parent,
                         out_node, blocked, (int)n_blocked, rows);
    };
    if (wide) {   // static LDS, one shape of workgroup
      launch(beam_expand_wide_kernel<kBlk, kFlt, kBia>, kWideThreads, 0);
    } else {
      launch(beam_expand_kernel<kBlk, kFlt, kBia>, kprev > 4 ? 64 * kExpMaxWaves : 64 * 4,
             beam_expand_lds(kprev, V, n_blocked, kBia));
    }
  });
  RQ_LAUNCH_CHECK(fn);
  return 0;
}

// rq_trie_allowed_nodes and rq_trie_bias_nodes: a per-group table (G, n_items) reduced onto the trie's D levels. The
// shared checks in one order and the levels struct filled (set_level: the entry point's own part), then the entry point's
// two launches through launch(kernel, work items, arguments...): its scatter (no items: no launch) and its finish.
static void set_level(AllowedLevels& lv, int64_t q, int32_t* bits, int64_t n_nodes) {
  lv.bits[q] = bits;
  lv.n_words[q] = (int)((n_nodes + 31) / 32);
}
static void set_level(BiasLevels& lv, int64_t q, float* upper, int64_t) { lv.upper[q] = reinterpret_cast<uint32_t*>(upper); }

template <typename Levels, typename Out, typename Launches>
static int trie_group_tables(const char* fn, const char* table_name, const void* table, int64_t G, int64_t n_items,
                             const int32_t* item_leaf, int64_t n_leaves, const int32_t* const* leaf_anc,
                             const int64_t* n_nodes, int64_t D, Out* const* out_levels, int64_t* out_leaf_item,
                             void* stream, Levels& lv, Launches launches) {
  RQ_CHECK_ARG(G >= 0 && D >= 1 && D <= RQ_BEAM_MAX_T, "%s: need G >= 0, 1 <= D <= %d (G=%lld, D=%lld)", fn,
               RQ_BEAM_MAX_T, (long long)G, (long long)D);
  RQ_CHECK_ARG(n_items >= 0 && n_leaves >= 0 && n_leaves < 0x7fffffff, "%s: bad corpus size", fn);
  RQ_CHECK_ARG(n_items == 0 || G <= INT64_MAX / 8 / n_items, "%s: %s too large", fn, table_name);
  RQ_CHECK_ARG(leaf_anc && n_nodes && out_levels, "%s: null level array", fn);
  for (int64_t q = 0; q < D; ++q) {
    RQ_CHECK_ARG(n_nodes[q] >= 0 && n_nodes[q] < 0x7fffffff, "%s: level %lld has %lld nodes", fn, (long long)(q + 1),
                 (long long)n_nodes[q]);
    RQ_CHECK_ARG((leaf_anc[q] || n_leaves == 0) && (out_levels[q] || n_nodes[q] == 0 || G == 0),
                 "%s: null table at level %lld", fn, (long long)(q + 1));
    lv.anc[q] = leaf_anc[q];
    lv.n_nodes[q] = (int)n_nodes[q];
    set_level(lv, q, out_levels[q], n_nodes[q]);
  }
  if (G == 0 || n_leaves == 0) return 0;
  RQ_CHECK_ARG(out_leaf_item && (n_items == 0 || (table && item_leaf)), "%s: null pointer", fn);
  launches([&](auto kernel, int64_t work, auto... args) {
    const int64_t blocks = std::min<int64_t>((work + kAllowThreads - 1) / kAllowThreads, kAllowMaxBlocks);
    if (blocks == 0) return;
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(kAllowThreads), 0, (hipStream_t)stream, args...);
  });
  RQ_LAUNCH_CHECK(fn);
  return 0;
}

}  // namespace rqhip

extern "C" {

using rqhip::AllowedBits, rqhip::BiasArgs, rqhip::arg_int;

int rq_beam_candidates(const float* logits, const float* noise, int64_t R, int64_t V, int64_t n_cand,
                       float temperature, int64_t* cand_ids, float* cand_lp, void* stream) {
  RQ_CHECK_ARG(R >= 0 && n_cand >= 1 && n_cand <= V && V <= rqhip::kBeamMaxV,
               "rq_beam_candidates: need R >= 0, 1 <= n_cand <= V <= %d (V=%lld, n_cand=%lld)", rqhip::kBeamMaxV,
               (long long)V, (long long)n_cand);
  RQ_CHECK_ARG(temperature > 0.f && temperature <= 3.0e38f, "rq_beam_candidates: temperature must be positive");
  if (R == 0) return 0;
  RQ_CHECK_ARG(logits && cand_ids && cand_lp, "rq_beam_candidates: null pointer");
  const int Vp = (int)((V + 3) / 4 * 4);
  const int waves = V <= 2048 ? 4 : 1;   // 2 Vp floats of LDS per wave, at most 64 KiB per workgroup
  const size_t lds = (size_t)waves * 2 * Vp * sizeof(float);
  const int64_t blocks = (R + waves - 1) / waves;
  RQ_CHECK_ARG(blocks <= 0x7fffffff, "rq_beam_candidates: too many rows");
  hipLaunchKernelGGL(rqhip::beam_candidates_kernel, dim3((unsigned)blocks), dim3(64 * waves), lds,
                     (hipStream_t)stream, logits, noise, R, (int)V, Vp, (int)n_cand, temperature, cand_ids, cand_lp);
  RQ_LAUNCH_CHECK("rq_beam_candidates");
  return 0;
}

int rq_beam_select_parent(const int64_t* cand_ids, const float* cand_lp, const bool* valid, const int64_t* keys,
                          int64_t n_keys, int64_t base, int64_t checked, const int64_t* parents,
                          const float* parent_lp, int64_t B, int64_t kprev, int64_t n_cand, int64_t P, int64_t k,
                          int64_t* out_ids, float* out_lp, int32_t* out_parent, void* stream) {
  RQ_CHECK_ARG(B >= 0 && kprev >= 1 && n_cand >= 1 && P >= 0 && P < 64, "rq_beam_select: bad shape");
  RQ_CHECK_ARG(kprev <= rqhip::kBeamMaxN && n_cand <= rqhip::kBeamMaxN && kprev * n_cand <= rqhip::kBeamMaxN &&
                   k >= 1 && k <= kprev * n_cand,
               "rq_beam_select: need 1 <= k <= kprev * n_cand <= %d (k=%lld, kprev=%lld, n_cand=%lld)",
               rqhip::kBeamMaxN, (long long)k, (long long)kprev, (long long)n_cand);
  RQ_CHECK_ARG((valid != nullptr) != (keys != nullptr), "rq_beam_select: give exactly one of valid and keys");
  RQ_CHECK_ARG((P == 0) ? (!parents && !parent_lp) : (parents && parent_lp),
               "rq_beam_select: parents and parent_lp are both NULL when P == 0, both given otherwise");
  if (keys) {
    RQ_CHECK_ARG(n_keys >= 0 && base >= 1 && checked >= 0, "rq_beam_select: bad key table");
    int64_t span = 1;   // base^(P+1) must fit an int64 (the packed key)
    for (int64_t j = 0; j <= P; ++j) {
      RQ_CHECK_ARG(span <= INT64_MAX / base, "rq_beam_select: base^(P+1) overflows int64 (base=%lld, P=%lld)",
                   (long long)base, (long long)P);
      span *= base;
    }
  }
  if (B == 0) return 0;
  RQ_CHECK_ARG(B <= 0x7fffffff, "rq_beam_select: too many batch elements");
  RQ_CHECK_ARG(cand_ids && cand_lp && out_ids && out_lp, "rq_beam_select: null pointer");
  const size_t lds = (size_t)((kprev * n_cand + 3) / 4 * 4 + 2 * (rqhip::kSelThreads / 64)) * sizeof(uint32_t);
  hipLaunchKernelGGL(rqhip::beam_select_kernel, dim3((unsigned)B), dim3(rqhip::kSelThreads), lds, (hipStream_t)stream,
                     cand_ids, cand_lp, valid, keys, n_keys, base, checked, parents, parent_lp, (int)kprev, (int)n_cand,
                     (int)P, (int)k, out_ids, out_lp, out_parent);
  RQ_LAUNCH_CHECK("rq_beam_select");
  return 0;
}

int rq_beam_select(const int64_t* cand_ids, const float* cand_lp, const bool* valid, const int64_t* keys,
                   int64_t n_keys, int64_t base, int64_t checked, const int64_t* parents, const float* parent_lp,
                   int64_t B, int64_t kprev, int64_t n_cand, int64_t P, int64_t k, int64_t* out_ids, float* out_lp,
                   void* stream) {
  return rq_beam_select_parent(cand_ids, cand_lp, valid, keys, n_keys, base, checked, parents, parent_lp, B, kprev,
                               n_cand, P, k, out_ids, out_lp, nullptr, stream);
}

int rq_beam_expand_biased(const float* logits, float temperature, const int32_t* node, const int32_t* child_off,
                          int64_t n_nodes, const int32_t* tok, int64_t n_children, const int64_t* parents,
                          const float* parent_lp, int64_t B, int64_t kprev, int64_t V, int64_t P, int64_t k,
                          int64_t* out_ids, float* out_lp, float* out_score, int32_t* out_parent, int32_t* out_node,
                          const int32_t* blocked, int64_t n_blocked, const float* bias, int64_t n_bias, int64_t G,
                          const int32_t* group, void* stream) {
  return rqhip::beam_expand_launch("rq_beam_expand_biased", false, logits, temperature, node, child_off, n_nodes, tok,
                            n_children, parents, parent_lp, B, kprev, V, P, k, out_ids, out_lp, out_parent, out_node,
                            blocked, n_blocked, BiasArgs{bias, group, arg_int(n_bias), arg_int(G), out_score}, stream);
}

int rq_beam_expand_wide_biased(const float* logits, float temperature, const int32_t* node, const int32_t* child_off,
                               int64_t n_nodes, const int32_t* tok, int64_t n_children, const int64_t* parents,
                               const float* parent_lp, int64_t B, int64_t kprev, int64_t V, int64_t P, int64_t k,
                               int64_t* out_ids, float* out_lp, float* out_score, int32_t* out_parent,
                               int32_t* out_node, const int32_t* blocked, int64_t n_blocked, const float* bias,
                               int64_t n_bias, int64_t G, const int32_t* group, void* stream) {
  return rqhip::beam_expand_launch("rq_beam_expand_wide_biased", true, logits, temperature, node, child_off, n_nodes, tok,
                            n_children, parents, parent_lp, B, kprev, V, P, k, out_ids, out_lp, out_parent, out_node,
                            blocked, n_blocked, BiasArgs{bias, group, arg_int(n_bias), arg_int(G), out_score}, stream);
}

int rq_beam_expand(const float* logits, float temperature, const int32_t* node, const int32_t* child_off,
                   int64_t n_nodes, const int32_t* tok, int64_t n_children, const int64_t* parents,
                   const float* parent_lp, int64_t B, int64_t kprev, int64_t V, int64_t P, int64_t k, int64_t* out_ids,
                   float* out_lp, int32_t* out_parent, int32_t* out_node, const int32_t* blocked, int64_t n_blocked,
                   const int32_t* allowed, int64_t n_words, int64_t G, const int32_t* group, void* stream) {
  return rqhip::beam_expand_launch("rq_beam_expand", false, logits, temperature, node, child_off, n_nodes, tok, n_children,
                            parents, parent_lp, B, kprev, V, P, k, out_ids, out_lp, out_parent, out_node, blocked,
                            n_blocked, AllowedBits{allowed, group, arg_int(n_words), arg_int(G)}, stream);
}

int rq_beam_expand_wide(const float* logits, float temperature, const int32_t* node, const int32_t* child_off,
                        int64_t n_nodes, const int32_t* tok, int64_t n_children, const int64_t* parents,
                        const float* parent_lp, int64_t B, int64_t kprev, int64_t V, int64_t P, int64_t k,
                        int64_t* out_ids, float* out_lp, int32_t* out_parent, int32_t* out_node,
                        const int32_t* blocked, int64_t n_blocked, const int32_t* allowed, int64_t n_words, int64_t G,
                        const int32_t* group, void* stream) {
  return rqhip::beam_expand_launch("rq_beam_expand_wide", true, logits, temperature, node, child_off, n_nodes, tok, n_children,
                            parents, parent_lp, B, kprev, V, P, k, out_ids, out_lp, out_parent, out_node, blocked,
                            n_blocked, AllowedBits{allowed, group, arg_int(n_words), arg_int(G)}, stream);
}

int rq_beam_expand_sampled(const float* logits, const float* noise, float temperature, const int32_t* node,
                           const int32_t* child_off, int64_t n_nodes, const int32_t* tok, int64_t n_children,
                           const int64_t* parents, const float* parent_phi, const float* parent_g, int64_t B,
                           int64_t kprev, int64_t V, int64_t P, int64_t k, int64_t* out_ids, float* out_phi,
                           float* out_g, int32_t* out_parent, int32_t* out_node, const int32_t* blocked,
                           int64_t n_blocked, const int32_t* allowed, int64_t n_words, int64_t G, const int32_t* group,
                           void* stream) {
  const char* fn = "rq_beam_expand_sampled";
  const AllowedBits ab = {allowed, group, arg_int(n_words), arg_int(G)};
  const int rc = rqhip::beam_expand_check(
      fn, rqhip::ExpandForm::kSampled, temperature, n_nodes, tok, n_children,
      (P == 0) ? (!node && !parents && !parent_phi && !parent_g) : (node && parents && parent_phi && parent_g),
      "node, parents, parent_phi and parent_g", B, kprev, V, P, k,
      logits && noise && child_off && out_ids && out_phi && out_g && out_parent && out_node, blocked, n_blocked, &ab);
  if (rc != 0 || B == 0) return rc;
  const rqhip::TrieLevel lvl = {child_off, (int)n_nodes, tok, (int)n_children};
  if (n_blocked == 0) blocked = nullptr;
  rqhip::with_tables(n_blocked > 0, ab, [&](auto blk, auto flt, auto) {
    hipLaunchKernelGGL((rqhip::beam_expand_sampled_kernel<decltype(blk)::value, decltype(flt)::value>),
                       dim3((unsigned)B), dim3(kprev > 4 ? 64 * rqhip::kExpMaxWaves : 64 * 4),
                       rqhip::beam_expand_lds(kprev, V, n_blocked, false), (hipStream_t)stream, logits, noise, temperature, node, lvl,
                       parents, parent_phi, parent_g, (int)kprev, (int)V, (int)P, (int)k, out_ids, out_phi, out_g,
                       out_parent, out_node, blocked, (int)n_blocked, ab);
  });
  RQ_LAUNCH_CHECK(fn);
  return 0;
}

int rq_score_paths(const float* logits, float temperature, const int64_t* tokens, int64_t tok_stride_b,
                   int64_t tok_stride_c, const bool* present, const float* prev_lp, int64_t B, int64_t C, int64_t V,
                   int64_t G, float* out_lp, int32_t* out_rank, void* stream) {
  RQ_CHECK_ARG(B >= 0 && V >= 1 && V <= rqhip::kBeamMaxV && C >= 1 && C <= rqhip::kRankMaxK && (G == 1 || G == C),
               "rq_score_paths: need B >= 0, 1 <= V <= %d, 1 <= C <= %d, G in {1, C} (V=%lld, C=%lld, G=%lld)",
               rqhip::kBeamMaxV, rqhip::kRankMaxK, (long long)V, (long long)C, (long long)G);
  RQ_CHECK_ARG(temperature > 0.f && temperature <= 3.0e38f, "rq_score_paths: temperature must be positive");
  RQ_CHECK_ARG(tok_stride_b >= 0 && tok_stride_c >= 0, "rq_score_paths: negative token stride");
  if (B == 0) return 0;
  RQ_CHECK_ARG(B <= 0x7fffffff, "rq_score_paths: too many batch elements");
  RQ_CHECK_ARG(logits && tokens && out_lp, "rq_score_paths: null pointer");
  hipStream_t hs = (hipStream_t)stream;
  if (V <= 256) {
    rqhip::launch_score_paths<4>(logits, temperature, tokens, tok_stride_b, tok_stride_c, present, prev_lp, B, (int)C,
                                 (int)V, (int)G, out_lp, out_rank, hs);
  } else if (V <= 1024) {
    rqhip::launch_score_paths<16>(logits, temperature, tokens, tok_stride_b, tok_stride_c, present, prev_lp, B, (int)C,
                                  (int)V, (int)G, out_lp, out_rank, hs);
  } else {
    rqhip::launch_score_paths<64>(logits, temperature, tokens, tok_stride_b, tok_stride_c, present, prev_lp, B, (int)C,
                                  (int)V, (int)G, out_lp, out_rank, hs);
  }
  RQ_LAUNCH_CHECK("rq_score_paths");
  return 0;
}

int rq_trie_blocked_nodes(const int64_t* items, int64_t B, int64_t H, const int32_t* item_leaf, int64_t n_items,
                          int64_t n_leaves, const int32_t* const* leaf_anc, const int32_t* const* leaf_count,
                          const int64_t* n_nodes, int64_t D, int32_t* out, void* stream) {
  RQ_CHECK_ARG(B >= 0 && H >= 0 && H <= rqhip::kBlockedMax && D >= 1 && D <= RQ_BEAM_MAX_T,
               "rq_trie_blocked_nodes: need B >= 0, 0 <= H <= %d, 1 <= D <= %d (H=%lld, D=%lld)", rqhip::kBlockedMax,
               RQ_BEAM_MAX_T, (long long)H, (long long)D);
  RQ_CHECK_ARG(n_items >= 0 && n_leaves >= 0 && n_leaves < 0x7fffffff, "rq_trie_blocked_nodes: bad corpus size");
  RQ_CHECK_ARG(leaf_anc && leaf_count && n_nodes, "rq_trie_blocked_nodes: null level array");
  rqhip::TrieLevels lv = {};
  for (int64_t q = 0; q < D; ++q) {
    RQ_CHECK_ARG(n_nodes[q] >= 0 && n_nodes[q] < 0x7fffffff, "rq_trie_blocked_nodes: level %lld has %lld nodes",
                 (long long)(q + 1), (long long)n_nodes[q]);
    RQ_CHECK_ARG((leaf_anc[q] || n_leaves == 0) && (leaf_count[q] || n_nodes[q] == 0),
                 "rq_trie_blocked_nodes: null table at level %lld", (long long)(q + 1));
    lv.anc[q] = leaf_anc[q];
    lv.cnt[q] = leaf_count[q];
    lv.n_nodes[q] = (int)n_nodes[q];
  }
  if (B == 0 || H == 0) return 0;
  RQ_CHECK_ARG(B <= 0x7fffffff, "rq_trie_blocked_nodes: too many batch elements");
  RQ_CHECK_ARG(items && out && (item_leaf || n_items == 0), "rq_trie_blocked_nodes: null pointer");
  int Hp = 1;
  while (Hp < H) Hp <<= 1;
  hipLaunchKernelGGL(rqhip::trie_blocked_kernel, dim3((unsigned)B), dim3(rqhip::kBlkThreads), 0, (hipStream_t)stream,
                     items, (int)H, Hp, item_leaf, n_items, (int)n_leaves, lv, (int)D, B, out);
  RQ_LAUNCH_CHECK("rq_trie_blocked_nodes");
  return 0;
}

int rq_trie_allowed_nodes(const bool* mask, int64_t G, int64_t n_items, const int32_t* item_leaf, int64_t n_leaves,
                          const int32_t* const* leaf_anc, const int64_t* n_nodes, int64_t D, int32_t* const* out_bits,
                          int64_t* out_leaf_item, void* stream) {
  rqhip::AllowedLevels lv = {};
  unsigned long long* lowest = reinterpret_cast<unsigned long long*>(out_leaf_item);
  return rqhip::trie_group_tables(
      "rq_trie_allowed_nodes", "mask", mask, G, n_items, item_leaf, n_leaves, leaf_anc, n_nodes, D, out_bits,
      out_leaf_item, stream, lv, [&](auto launch) {
        launch(rqhip::trie_allowed_kernel, (G * n_items + 3) / 4, reinterpret_cast<const uint8_t*>(mask), G, n_items,
               item_leaf, (int)n_leaves, lv, (int)D, lowest);
        launch(rqhip::trie_allowed_finish_kernel, G * n_leaves, lowest, G * n_leaves);
      });
}

int rq_trie_bias_nodes(const float* bias, int64_t G, int64_t n_items, const int32_t* item_leaf, int64_t n_leaves,
                       const int32_t* const* leaf_anc, const int64_t* n_nodes, int64_t D, float* const* out_upper,
                       int64_t* out_leaf_item, void* stream) {
  // its own two: the scatter packs an item index into 32 bits of a key, the finish indexes the (group, leaf) pairs
  RQ_CHECK_ARG(n_items <= 0x7fffffff, "rq_trie_bias_nodes: bad corpus size");
  RQ_CHECK_ARG(n_leaves <= 0 || G <= INT64_MAX / 8 / n_leaves, "rq_trie_bias_nodes: too many (group, leaf) pairs");
  rqhip::BiasLevels lv = {};
  unsigned long long* best = reinterpret_cast<unsigned long long*>(out_leaf_item);
  return rqhip::trie_group_tables(
      "rq_trie_bias_nodes", "bias", bias, G, n_items, item_leaf, n_leaves, leaf_anc, n_nodes, D, out_upper,
      out_leaf_item, stream, lv, [&](auto launch) {
        launch(rqhip::trie_bias_kernel, G * n_items, bias, G, n_items, item_leaf, (int)n_leaves, lv, (int)D, best);
        launch(rqhip::trie_bias_finish_kernel, G * n_leaves, lv, (int)D, G, best, G * n_leaves);
      });
}

int rq_beam_self_attn(const float* q, int64_t sq, const float* const* k_steps, const float* const* v_steps,
                      const int64_t* strides, const int64_t* rows, const int32_t* anc, int64_t R, int64_t t,
                      int64_t H, int64_t hd, float scale, float* out, int64_t so, void* stream) {
  RQ_CHECK_ARG(R >= 0 && t >= 0 && t < RQ_BEAM_MAX_T && H >= 1 && H <= 4096,
               "rq_beam_self_attn: need R >= 0, 0 <= t < %d, 1 <= H <= 4096 (R=%lld, t=%lld, H=%lld)", RQ_BEAM_MAX_T,
               (long long)R, (long long)t, (long long)H);
  RQ_CHECK_ARG(hd == 16 || hd == 32 || hd == 64 || hd == 128, "rq_beam_self_attn: head_dim must be 16, 32, 64 or 128 (got %lld)",
               (long long)hd);
  const int64_t A = H * hd;
  RQ_CHECK_ARG(sq >= A && sq % 4 == 0 && so >= A && so % 4 == 0,
               "rq_beam_self_attn: q / out row strides must be >= H * hd and multiples of 4");
  RQ_CHECK_ARG(k_steps && v_steps && strides && rows, "rq_beam_self_attn: null step array");
  RQ_CHECK_ARG((anc == nullptr) == (t == 0), "rq_beam_self_attn: anc is NULL exactly when t == 0");
  rqhip::BeamSteps st = {};
  for (int64_t s = 0; s <= t; ++s) {
    RQ_CHECK_ARG(rows[s] >= (R > 0 ? 1 : 0) && rows[s] <= 0x7fffffff, "rq_beam_self_attn: step %lld has %lld rows",
                 (long long)s, (long long)rows[s]);
    RQ_CHECK_ARG(strides[s] >= A && strides[s] % 4 == 0,
                 "rq_beam_self_attn: step %lld row stride %lld must be >= H * hd and a multiple of 4", (long long)s,
                 (long long)strides[s]);
    RQ_CHECK_ARG(R == 0 || (k_steps[s] && v_steps[s]), "rq_beam_self_attn: null K / V pointer at step %lld", (long long)s);
    RQ_CHECK_ARG(((uintptr_t)k_steps[s] | (uintptr_t)v_steps[s]) % 16 == 0,
                 "rq_beam_self_attn: K / V of step %lld must be 16-byte aligned", (long long)s);
    st.k[s] = k_steps[s];
    st.v[s] = v_steps[s];
    st.stride[s] = strides[s];
    st.rows[s] = rows[s];
  }
  RQ_CHECK_ARG(rows[t] == R, "rq_beam_self_attn: the current step holds one row per beam (rows[t]=%lld, R=%lld)",
               (long long)rows[t], (long long)R);
  if (R == 0) return 0;
  RQ_CHECK_ARG(q && out, "rq_beam_self_attn: null pointer");
  RQ_CHECK_ARG(((uintptr_t)q | (uintptr_t)out) % 16 == 0, "rq_beam_self_attn: q / out must be 16-byte aligned");
  const int64_t units = R * H;
  RQ_CHECK_ARG(units <= ((int64_t)1 << 33), "rq_beam_self_attn: too many (row, head) units");
  hipStream_t hs = (hipStream_t)stream;
  switch (hd) {
    case 16: rqhip::launch_beam_self_attn<4>(q, sq, st, anc, units, (int)H, (int)t, scale, out, so, hs); break;
    case 32: rqhip::launch_beam_self_attn<8>(q, sq, st, anc, units, (int)H, (int)t, scale, out, so, hs); break;
    case 64: rqhip::launch_beam_self_attn<16>(q, sq, st, anc, units, (int)H, (int)t, scale, out, so, hs); break;
    default: rqhip::launch_beam_self_attn<32>(q, sq, st, anc, units, (int)H, (int)t, scale, out, so, hs); break;
  }
  RQ_LAUNCH_CHECK("rq_beam_self_attn");
  return 0;
}

int rq_topk_hits(const int64_t* actual, const int64_t* topk, int64_t B, int64_t k, int64_t D, const int* ks,
                 int64_t n_ks, int64_t* counts, void* stream) {
  RQ_CHECK_ARG(B >= 0 && k >= 1 && k <= 0x3fffffff && D >= 1 && D <= rqhip::kHitsMaxD && n_ks >= 1 &&
                   n_ks <= rqhip::kHitsMaxKs,
               "rq_topk_hits: need k >= 1, 1 <= D <= %d, 1 <= n_ks <= %d", rqhip::kHitsMaxD, rqhip::kHitsMaxKs);
  RQ_CHECK_ARG(ks, "rq_topk_hits: null pointer");
  if (B == 0) return 0;
  RQ_CHECK_ARG(actual && topk && counts, "rq_topk_hits: null pointer");
  rqhip::HitKs h;
  for (int j = 0; j < rqhip::kHitsMaxKs; ++j) h.v[j] = j < n_ks ? ks[j] : 0;
  const int64_t blocks = std::min<int64_t>((B + 3) / 4, 1024);
  hipLaunchKernelGGL(rqhip::topk_hits_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, actual, topk,
                     B, (int)k, (int)D, h, (int)n_ks, reinterpret_cast<unsigned long long*>(counts));
  RQ_LAUNCH_CHECK("rq_topk_hits");
  return 0;
}

int rq_rank_hist(const int64_t* actual, const int64_t* topk, int64_t B, int64_t k, int64_t D, int64_t* hist,
                 void* stream) {
  RQ_CHECK_ARG(B >= 0 && k >= 1 && k <= rqhip::kRankMaxK && D >= 1 && D <= rqhip::kHitsMaxD,
               "rq_rank_hist: need 1 <= k <= %d, 1 <= D <= %d (k=%lld, D=%lld)", rqhip::kRankMaxK, rqhip::kHitsMaxD,
               (long long)k, (long long)D);
  if (B == 0) return 0;
  RQ_CHECK_ARG(actual && topk && hist, "rq_rank_hist: null pointer");
  const int64_t blocks = std::min<int64_t>((B + 3) / 4, 1024);
  hipLaunchKernelGGL(rqhip::rank_hist_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, actual, topk, B,
                     (int)k, (int)D, reinterpret_cast<unsigned long long*>(hist));
  RQ_LAUNCH_CHECK("rq_rank_hist");
  return 0;
}

}  // extern "C"
