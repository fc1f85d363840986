// Codebook usage counters, dead-code revival and EMA-maintained codebooks (statistics + update, below) for the
// RQ-VAE tokenizer.
//
// Extensions: the reference only LOGS codebook usage at checkpoint time (train_rqvae.py:232-239,
// `codebook_usage_{l}` = len(unique(corpus_ids[:, l])) / K) and has no countermeasure against codebook
// collapse beyond its one-shot k-means init. Here the usage is counted on the device inside the training
// step (rq_code_usage: one launch, integer atomics only, graph-capturable), and codewords that nothing
// selected are re-seated on encoder residuals of the data (rq_codebook_revive) by a rule that only copies
// and zeroes, so every data-parallel rank and the CPU restatement reproduce it bit for bit:
//
//   dead codes of level l = {k : counts[l][k] < min_count}, ascending k; the j-th of them takes donor row
//   r = (s_l + j) mod B of res[l], s_l = splitmix64(seed, l) mod B; codebook_l[k] = res[l][r] (bit copy),
//   both AdamW moment rows of k become +0.0, revived[l][k] = 1, n_revived[l] = #dead. B >= K, so the
//   donors of a level are distinct rows.
#include "common.h"

namespace rqhip {

// ------------------------------------------------------------------------------------------- usage
constexpr int kUsageLdsBins = 8192;    // L K up to here: histogram privatised in LDS (32 KiB of uint32)
constexpr int kUsageMaxBlocks = 1024;  // grid cap of the grid-stride loop
constexpr int kUsagePeel = 4;          // LDS path: hot bins aggregated per wave before the per-lane adds

// One wave adds 1 to bin[lane] for every lane with bin >= 0. Lanes that share a bin are aggregated: the
// lowest pending lane's bin is broadcast, every lane holding it retires, and that lane adds their number
// once. A collapsed codebook (thousands of rows on one bin per level) therefore costs one add per level
// and wave, not 64 serialised ones. After `rounds` rounds the lanes still pending (`rest`) are the
// caller's: the LDS path adds them one by one (LDS atomics on distinct bins do not serialise), the global
// path passes rounds = 64 and is left with none. Must be called by all 64 lanes.
template <typename Add>
__device__ __forceinline__ uint64_t wave_aggregate(int bin, int rounds, Add add) {
  const int lane = (int)(threadIdx.x & 63);
  uint64_t todo = __ballot(bin >= 0);
  for (int it = 0; it < rounds && todo != 0; ++it) {   // wave-uniform condition
    const int lead = __ffsll((unsigned long long)todo) - 1;
    const int b0 = __shfl(bin, lead, 64);
    const uint64_t same = __ballot(bin == b0);   // b0 >= 0: only pending lanes match
    if (lane == lead) add(b0, (unsigned)__popcll(same));
    todo &= ~same;
  }
  return todo;
}

// bin of flat element e of ids (B, L): level e % L, code ids[e]; -1 for ids outside [0, K) and e >= n.
__device__ __forceinline__ int usage_bin(const int64_t* __restrict__ ids, int64_t e, int64_t n, int64_t L, int64_t K) {
  if (e >= n) return -1;
  const int64_t k = ids[e];
  if (k < 0 || k >= K) return -1;
  return (int)((e % L) * K + k);
}

template <bool kLds>
__global__ void __launch_bounds__(256) code_usage_kernel(const int64_t* __restrict__ ids, int64_t n, int64_t L, int64_t K,
                                                         unsigned long long* __restrict__ counts) {
  __shared__ unsigned s_hist[kLds ? kUsageLdsBins : 1];
  const int bins = (int)(L * K);
  if (kLds) {
    for (int i = threadIdx.x; i < bins; i += 256) s_hist[i] = 0u;
    __syncthreads();
  }
  const int lane = (int)(threadIdx.x & 63);
  const int64_t stride = (int64_t)gridDim.x * 256;
  // the loop bound is uniform over the wave (base is the wave's lane-0 element): every lane reaches the ballots
  for (int64_t base = (int64_t)blockIdx.x * 256 + (threadIdx.x & ~63u); base < n; base += stride) {
    const int bin = usage_bin(ids, base + lane, n, L, K);
    if (kLds) {
      const uint64_t rest = wave_aggregate(bin, kUsagePeel, [&](int b, unsigned c) { atomicAdd(&s_hist[b], c); });
      if ((rest >> lane) & 1) atomicAdd(&s_hist[bin], 1u);
    } else {
      wave_aggregate(bin, 64, [&](int b, unsigned c) { atomicAdd(&counts[b], (unsigned long long)c); });
    }
  }
  if (kLds) {
    __syncthreads();
    for (int i = threadIdx.x; i < bins; i += 256) {   // one 64-bit add per non-zero bin per workgroup
      const unsigned c = s_hist[i];
      if (c != 0u) atomicAdd(&counts[i], (unsigned long long)c);
    }
  }
}

// ------------------------------------------------------------------------------------------ revive
constexpr int kReviveMaxL = 16;
constexpr int kReviveChunk = 256;   // codes per workgroup = threads per workgroup

struct ReviveTable {   // BY VALUE in the kernel arguments (384 B), as rq_adamw_step's segment table
  float* cb[kReviveMaxL];
  float* m[kReviveMaxL];
  float* v[kReviveMaxL];
};

// Dead flag of this thread's code and its exclusive rank among the workgroup's dead codes; *total = their number.
__device__ __forceinline__ int chunk_rank(bool dead, int* total) {
  __shared__ int s_wave[kReviveChunk / 64];
  const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
  const uint64_t mask = __ballot(dead);
  if (lane == 0) s_wave[wave] = __popcll(mask);
  __syncthreads();
  int before = 0, all = 0;
#pragma unroll
  for (int w = 0; w < kReviveChunk / 64; ++w) {
    before += w < wave ? s_wave[w] : 0;
    all += s_wave[w];
  }
  *total = all;
  return before + __popcll(mask & ((1ull << lane) - 1ull));
}

// Launch 1: grid (chunks, L). revived[l][k] and the chunk's dead total -> chunk_tot[l][chunk].
__global__ void __launch_bounds__(kReviveChunk) revive_mark_kernel(const int64_t* __restrict__ counts, int64_t K,
                                                                   int64_t min_count, uint8_t* __restrict__ revived,
                                                                   int* __restrict__ chunk_tot) {
  const int64_t l = blockIdx.y, k = (int64_t)blockIdx.x * kReviveChunk + threadIdx.x;
  const bool dead = k < K && counts[l * K + k] < min_count;
  if (k < K) revived[l * K + k] = dead ? 1 : 0;
  int total;
  chunk_rank(dead, &total);
  if (threadIdx.x == 0) chunk_tot[l * gridDim.x + blockIdx.x] = total;
}

// Launch 2: grid (chunks, L). The rank of the chunk's first dead code is the sum of the earlier chunks'
// totals (at most 4096 ints per level, 16 per thread: the counts themselves are not rescanned); then one
// wave per dead code copies the donor row and zeroes the moment rows, 16 bytes per lane.
__global__ void __launch_bounds__(kReviveChunk) revive_copy_kernel(const ReviveTable tab, const int64_t* __restrict__ counts,
                                                                   int64_t K, int64_t D, int64_t min_count,
                                                                   const float* __restrict__ res, int64_t B, uint64_t seed,
                                                                   const int* __restrict__ chunk_tot,
                                                                   int64_t* __restrict__ n_revived) {
  __shared__ int s_pre[kReviveChunk / 64], s_all[kReviveChunk / 64];
  __shared__ int s_code[kReviveChunk];   // local index of the chunk's j-th dead code
  const int l = (int)blockIdx.y, chunk = (int)blockIdx.x, nchunks = (int)gridDim.x;
  const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
  int pre = 0, all = 0;
  for (int c = threadIdx.x; c < nchunks; c += kReviveChunk) {
    const int t = chunk_tot[l * nchunks + c];
    pre += c < chunk ? t : 0;
    all += t;
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    pre += __shfl_xor(pre, o, 64);
    all += __shfl_xor(all, o, 64);
  }
  if (lane == 0) { s_pre[wave] = pre; s_all[wave] = all; }
  __syncthreads();
  pre = 0, all = 0;
#pragma unroll
  for (int w = 0; w < kReviveChunk / 64; ++w) { pre += s_pre[w]; all += s_all[w]; }
  if (chunk == 0 && threadIdx.x == 0) n_revived[l] = all;

  const int64_t k = (int64_t)chunk * kReviveChunk + threadIdx.x;
  const bool dead = k < K && counts[(int64_t)l * K + k] < min_count;
  int ndead;
  const int j = chunk_rank(dead, &ndead);
  if (dead) s_code[j] = (int)threadIdx.x;
  __syncthreads();
  if (ndead == 0) return;

  const uint64_t s_l = splitmix64(seed, (uint64_t)l) % (uint64_t)B;
  float* __restrict__ cb = tab.cb[l];
  float* __restrict__ m = tab.m[l];
  float* __restrict__ v = tab.v[l];
  const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int i = wave; i < ndead; i += kReviveChunk / 64) {
    const int64_t code = (int64_t)chunk * kReviveChunk + s_code[i];
    uint64_t r = s_l + (uint64_t)(pre + i);   // s_l < B and rank < K <= B: below 2 B
    if (r >= (uint64_t)B) r -= (uint64_t)B;
    const float* __restrict__ src = res + ((int64_t)l * B + (int64_t)r) * D;
    for (int64_t d = 4 * lane; d < D; d += 256) {
      *reinterpret_cast<float4*>(cb + code * D + d) = *reinterpret_cast<const float4*>(src + d);
      if (m != nullptr) {
        *reinterpret_cast<float4*>(m + code * D + d) = zero;
        *reinterpret_cast<float4*>(v + code * D + d) = zero;
      }
    }
  }
}

static inline int64_t revive_chunks(int64_t K) { return (K + kReviveChunk - 1) / kReviveChunk; }

// --------------------------------------------------------------------------------- EMA statistics
// Per-code statistics of a batch for EMA-maintained codebooks (an extension; rule in include/rqvae_hip.h):
// n[l][k] += #{b : ids[b][l] == k}, s[l][k] += sum of those rows of res[l], no float atomics.
// Workgroup (c, l, t) owns the rows [c R, (c + 1) R) of level l and the codes [t KT, (t + 1) KT), whose sums it
// keeps in an LDS image acc[KT][D]. It walks its rows in sub-blocks of kEmaRows ids held in LDS; wave w of 16 owns
// the tile's codes k with 16 k / KT' == w (KT' = the tile's code count) and collects its matching rows in
// ascending order (a ballot per 64 rows, as rq_cb_chunk_kernel). A row is G = D / 4 (rounded up to a power of
// two, at most 64) lanes wide, so one wave load fetches 64 / G matches; they are then added into the image one
// match at a time, lowest row first (LDS operations of one wave execute in program order), so every acc[k] is a
// row-ordered sum whatever the other waves do. Counts are LDS integer adds by the owning wave. The image and the
// counts go to partial[l][c]; ema_stats_reduce adds the chunks in c order (slab_sum_w4) into s and n.
constexpr int kEmaRows = 1024;       // ids per sub-block
constexpr int kEmaWaves = 16;
constexpr int kEmaList = 256;        // match-list entries per wave
constexpr int kEmaMaxChunks = 64;    // row chunks per level, at most
constexpr int kEmaMaxTile = 2048;    // codes per tile, at most (their LDS counters)
constexpr int64_t kEmaPartialElems = 1ll << 22;   // K D chunks <= this (or one chunk): bounds the workspace

struct EmaPlan {
  int form, chunks, tiles, kt;
  int64_t rows;
  size_t lds;
};

static EmaPlan ema_plan(int64_t B, int64_t D, int64_t K) {
  EmaPlan p = {RQ_EMA_STATS_NONE, 0, 0, 0, 0, 0};
  if (B == 0) return p;
  p.kt = (int)std::min<int64_t>(std::min<int64_t>(K, RQ_EMA_STATS_LDS_ELEMS / D), kEmaMaxTile);
  p.tiles = (int)((K + p.kt - 1) / p.kt);
  p.form = p.tiles == 1 ? RQ_EMA_STATS_LDS : RQ_EMA_STATS_TILED;
  const int64_t max_chunks = std::max<int64_t>(1, std::min<int64_t>(kEmaMaxChunks, kEmaPartialElems / (K * D)));
  const int64_t blocks = (B + kEmaRows - 1) / kEmaRows;
  const int64_t per = (blocks + max_chunks - 1) / max_chunks;   // sub-blocks per chunk
  p.chunks = (int)((blocks + per - 1) / per);
  p.rows = per * kEmaRows;
  p.lds = (size_t)p.kt * D * sizeof(float) + (size_t)p.kt * sizeof(int) + kEmaRows * sizeof(int) +
          kEmaWaves * kEmaList * sizeof(unsigned short);
  return p;
}

__global__ void __launch_bounds__(64 * kEmaWaves) ema_stats_kernel(const float* __restrict__ res,
                                                                   const int64_t* __restrict__ ids, int64_t B, int D, int K,
                                                                   int L, int KT, int64_t rows, float* __restrict__ part_s,
                                                                   int* __restrict__ part_n) {
  extern __shared__ __attribute__((aligned(16))) float acc[];   // [KT][D], counts, the sub-block's ids, match lists
  int* cnt = reinterpret_cast<int*>(acc + (int64_t)KT * D);
  int* ids_s = cnt + KT;
  const int c = blockIdx.x, l = blockIdx.y, t = blockIdx.z, nchunk = gridDim.x, tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  unsigned short* list = reinterpret_cast<unsigned short*>(ids_s + kEmaRows) + wave * kEmaList;
  const int k0 = t * KT, kn = min(KT, K - k0), D4 = D / 4;
  int G = 1;
  while (G < D4 && G < 64) G <<= 1;
  const int NR = 64 / G, g = lane / G, col0 = lane & (G - 1);
  for (int i = tid; i < kn * D4; i += 64 * kEmaWaves) reinterpret_cast<float4*>(acc)[i] = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int i = tid; i < kn; i += 64 * kEmaWaves) cnt[i] = 0;
  const int64_t rbeg = (int64_t)c * rows, rend = min(B, rbeg + rows);
  const float* xl = res + (int64_t)l * B * D;
  for (int64_t sb = rbeg; sb < rend; sb += kEmaRows) {   // uniform over the workgroup
    __syncthreads();   // the image is zeroed / the previous sub-block's ids are consumed
    for (int i = tid; i < kEmaRows; i += 64 * kEmaWaves) {
      const int64_t r = sb + i;
      const int64_t k = r < rend ? ids[r * L + l] : -1;
      ids_s[i] = (k >= k0 && k < (int64_t)k0 + kn) ? (int)(k - k0) : -1;   // k0 >= 0, k0 + kn <= K
    }
    __syncthreads();
    // this wave's matches (list entries i0 ..), 64 / G at a time: loads first, then the row-ordered adds
    auto drain = [&](int n_list) {
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // the list entries other lanes wrote
      for (int i0 = 0; i0 < n_list; i0 += NR) {
        // unconditional loads (lanes past the list repeat its last entry, columns past the row its last column;
        // neither is added): a branch around a load makes the compiler wait for it at the merge
        const int row = list[min(i0 + g, n_list - 1)];
        const int kc = ids_s[row];
        const float4* __restrict__ src = reinterpret_cast<const float4*>(xl + (sb + row) * D);
        float4 v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = src[min(col0 + 64 * j, D4 - 1)];
        float4* a = reinterpret_cast<float4*>(acc + (int64_t)kc * D);
        const int nb = min(NR, n_list - i0);
        for (int u = 0; u < nb; ++u) {
          if (g == u) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              const int col = col0 + 64 * j;
              if (col < D4) {
                float4 o = a[col];
                o.x += v[j].x; o.y += v[j].y; o.z += v[j].z; o.w += v[j].w;
                a[col] = o;
              }
            }
          }
        }
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // the list is rewritten after this
    };
    const int nrows = (int)min((int64_t)kEmaRows, rend - sb);
    int n_list = 0;
    for (int g0 = 0; g0 < nrows; g0 += 64) {
      const int kk = ids_s[g0 + lane];
      const bool mine = kk >= 0 && (kEmaWaves * kk) / kn == wave;
      const unsigned long long m = __ballot(mine);
      const int n_mine = __popcll(m);
      if (n_list + n_mine > kEmaList) {
        drain(n_list);
        n_list = 0;
      }
      const int before = __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
      if (mine) {
        list[n_list + before] = (unsigned short)(g0 + lane);
        atomicAdd(&cnt[kk], 1);   // only this wave touches cnt[kk]; lanes may share kk
      }
      n_list += n_mine;
    }
    drain(n_list);
  }
  __syncthreads();
  const int64_t slot = (int64_t)l * nchunk + c;
  float4* dst = reinterpret_cast<float4*>(part_s + (slot * K + k0) * D);
  for (int i = tid; i < kn * D4; i += 64 * kEmaWaves) dst[i] = reinterpret_cast<const float4*>(acc)[i];
  for (int i = tid; i < kn; i += 64 * kEmaWaves) part_n[slot * K + k0 + i] = cnt[i];
}

// s[l][j] = s[l][j] + (sum over chunks c, in order, of part_s[l][c][j]); n[l][k] += sum over c of part_n[l][c][k].
__global__ void __launch_bounds__(256) ema_stats_reduce_kernel(const float* __restrict__ part_s,
                                                               const int* __restrict__ part_n, int nchunk, int64_t K,
                                                               int64_t KD, float* __restrict__ s, int64_t* __restrict__ n) {
  const int l = blockIdx.y;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x, j = 4 * i;
  if (j < KD) {
    const float4 r = slab_sum_w4(part_s + (int64_t)l * nchunk * KD, nchunk, KD, j);
    float4* o = reinterpret_cast<float4*>(s + (int64_t)l * KD + j);
    float4 v = *o;
    v.x += r.x; v.y += r.y; v.z += r.z; v.w += r.w;
    *o = v;
  }
  if (i < K) {   // K <= K D / 4: the grid covers every code
    // eight loads in flight per round (indices past the end re-read the last chunk and are not added), as
    // strided_slab_sum: one dependent load per chunk made this the longest thread of the launch
    const int* __restrict__ p = part_n + (int64_t)l * nchunk * K + i;
    int64_t total = 0;
    for (int c = 0; c < nchunk; c += 8) {
      int v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = p[(int64_t)min(c + u, nchunk - 1) * K];
#pragma unroll
      for (int u = 0; u < 8; ++u)
        if (c + u < nchunk) total += v[u];
    }
    n[(int64_t)l * K + i] += total;
  }
}

// ------------------------------------------------------------------------------------- EMA update
struct EmaTable {   // BY VALUE in the kernel arguments
  float* cb[kReviveMaxL];
};

// One workgroup per level: another workgroup of the level would read N while this one rewrites it. Pass 1 writes
// N' = g N + (1 - g) n, zeroes n and sums T = sum_k N' (per-thread strided sums, a butterfly per wave, the 16 wave
// sums in wave order: a fixed order); pass 2 writes S', zeroes s and writes the codewords S' / N~.
constexpr int kEmaApplyThreads = 1024;
__global__ void __launch_bounds__(kEmaApplyThreads) ema_apply_kernel(const EmaTable tab, int K, int D, float* __restrict__ N,
                                                                     float* __restrict__ S, int64_t* __restrict__ n,
                                                                     float* __restrict__ s, float g, float omg, float eps,
                                                                     float keps) {
  __shared__ float s_wave[kEmaApplyThreads / 64];
  const int l = blockIdx.x, tid = threadIdx.x;
  float* __restrict__ Nl = N + (int64_t)l * K;
  int64_t* __restrict__ nl = n + (int64_t)l * K;
  float part = 0.f;
  for (int k = tid; k < K; k += kEmaApplyThreads) {
    const float np = g * Nl[k] + omg * (float)nl[k];
    Nl[k] = np;
    nl[k] = 0;
    part += np;
  }
  part = group_sum<64>(part);
  if ((tid & 63) == 0) s_wave[tid >> 6] = part;
  __syncthreads();   // also: every N' of the level is written
  float T = 0.f;
#pragma unroll
  for (int w = 0; w < kEmaApplyThreads / 64; ++w) T += s_wave[w];
  const float den = T + keps;
  const int D4 = D / 4;
  float4* __restrict__ Sl = reinterpret_cast<float4*>(S + (int64_t)l * K * D);
  float4* __restrict__ sl = reinterpret_cast<float4*>(s + (int64_t)l * K * D);
  float4* __restrict__ W = reinterpret_cast<float4*>(tab.cb[l]);
  for (int e = tid; e < K * D4; e += kEmaApplyThreads) {
    const float nt = (Nl[e / D4] + eps) / den * T;
    const float4 a = Sl[e], b = sl[e];
    const float4 sp = make_float4(g * a.x + omg * b.x, g * a.y + omg * b.y, g * a.z + omg * b.z, g * a.w + omg * b.w);
    Sl[e] = sp;
    sl[e] = make_float4(0.f, 0.f, 0.f, 0.f);
    W[e] = make_float4(sp.x / nt, sp.y / nt, sp.z / nt, sp.w / nt);
  }
}

static bool ema_shape_ok(int64_t B, int64_t D, int64_t K, int64_t L) {
  return L >= 1 && L <= kReviveMaxL && K >= 1 && K <= 4096 && D >= 4 && D % 4 == 0 && D <= 1024 && B >= 0 &&
         B < (1ll << 31);
}

}  // namespace rqhip

using namespace rqhip;

extern "C" {

int rq_code_usage(const int64_t* ids, int64_t B, int64_t L, int64_t K, int64_t* counts, void* stream) {
  RQ_CHECK_ARG(B >= 0 && L >= 1 && K >= 1, "rq_code_usage: need B >= 0, L >= 1, K >= 1 (B=%lld L=%lld K=%lld)",
               (long long)B, (long long)L, (long long)K);
  RQ_CHECK_ARG(K <= (1ll << 30) && L <= (1ll << 30) && L * K < (1ll << 31), "rq_code_usage: L K must be below 2^31");
  RQ_CHECK_ARG(B <= (1ll << 40) / L, "rq_code_usage: B L must be at most 2^40");
  if (B == 0) return 0;
  RQ_CHECK_ARG(ids != nullptr && counts != nullptr, "rq_code_usage: null pointer");
  const int64_t n = B * L, bins = L * K;
  const bool lds = bins <= kUsageLdsBins;
  // a workgroup zeroes and flushes `bins` LDS counters: give it enough elements to pay for them
  const int64_t per_block = lds ? std::max<int64_t>(4096, 4 * bins) : 4096;
  const int64_t blocks = std::min<int64_t>(kUsageMaxBlocks, (n + per_block - 1) / per_block);
  unsigned long long* c = reinterpret_cast<unsigned long long*>(counts);
  if (lds)
    hipLaunchKernelGGL(code_usage_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, ids, n, L, K, c);
  else
    hipLaunchKernelGGL(code_usage_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, ids, n, L, K, c);
  RQ_LAUNCH_CHECK("rq_code_usage");
  return 0;
}

size_t rq_codebook_revive_workspace(int64_t L, int64_t K) {
  if (L < 1 || L > kReviveMaxL || K < 1 || K > (1ll << 20)) return 0;
  return (size_t)(L * revive_chunks(K)) * sizeof(int);
}

int rq_codebook_revive(float* const* codebooks, float* const* exp_avg, float* const* exp_avg_sq, int64_t L, int64_t K,
                       int64_t D, const int64_t* counts, int64_t min_count, const float* res, int64_t B, uint64_t seed,
                       uint8_t* revived, int64_t* n_revived, void* workspace, size_t ws_bytes, void* stream) {
  RQ_CHECK_ARG(L >= 1 && L <= kReviveMaxL, "rq_codebook_revive: need 1 <= L <= %d (L=%lld)", kReviveMaxL, (long long)L);
  RQ_CHECK_ARG(K >= 1 && K <= (1ll << 20), "rq_codebook_revive: need 1 <= K <= 2^20 (K=%lld)", (long long)K);
  RQ_CHECK_ARG(D >= 4 && D % 4 == 0 && D <= 1024, "rq_codebook_revive: need D %% 4 == 0 and 4 <= D <= 1024 (D=%lld)",
               (long long)D);
  RQ_CHECK_ARG(min_count >= 0, "rq_codebook_revive: min_count < 0");
  RQ_CHECK_ARG(B >= K, "rq_codebook_revive: need B >= K donor rows per level (B=%lld, K=%lld)", (long long)B,
               (long long)K);
  RQ_CHECK_ARG(codebooks && counts && res && revived && n_revived, "rq_codebook_revive: null pointer");
  RQ_CHECK_ARG((exp_avg == nullptr) == (exp_avg_sq == nullptr),
               "rq_codebook_revive: exp_avg and exp_avg_sq go together (both or neither)");
  RQ_CHECK_ARG((uintptr_t)res % 16 == 0, "rq_codebook_revive: res must be 16-byte aligned");
  ReviveTable tab;
  for (int l = 0; l < kReviveMaxL; ++l) {
    tab.cb[l] = l < L ? codebooks[l] : nullptr;
    tab.m[l] = (l < L && exp_avg) ? exp_avg[l] : nullptr;
    tab.v[l] = (l < L && exp_avg_sq) ? exp_avg_sq[l] : nullptr;
    if (l >= L) continue;
    RQ_CHECK_ARG(tab.cb[l] != nullptr && (uintptr_t)tab.cb[l] % 16 == 0,
                 "rq_codebook_revive: codebook %d is null or not 16-byte aligned", l);
    if (exp_avg)
      RQ_CHECK_ARG(tab.m[l] && tab.v[l] && (uintptr_t)tab.m[l] % 16 == 0 && (uintptr_t)tab.v[l] % 16 == 0,
                   "rq_codebook_revive: moments of level %d are null or not 16-byte aligned", l);
  }
  const size_t need = rq_codebook_revive_workspace(L, K);
  RQ_CHECK_ARG(workspace != nullptr && ws_bytes >= need && (uintptr_t)workspace % 4 == 0,
               "rq_codebook_revive: workspace too small or misaligned (%zu < %zu bytes)", ws_bytes, need);
  const dim3 grid((unsigned)revive_chunks(K), (unsigned)L);
  int* chunk_tot = reinterpret_cast<int*>(workspace);
  hipLaunchKernelGGL(revive_mark_kernel, grid, dim3(kReviveChunk), 0, (hipStream_t)stream, counts, K, min_count, revived,
                     chunk_tot);
  RQ_LAUNCH_CHECK("rq_codebook_revive (mark)");
  hipLaunchKernelGGL(revive_copy_kernel, grid, dim3(kReviveChunk), 0, (hipStream_t)stream, tab, counts, K, D, min_count,
                     res, B, seed, chunk_tot, n_revived);
  RQ_LAUNCH_CHECK("rq_codebook_revive (copy)");
  return 0;
}

int rq_codebook_ema_stats_plan(int64_t B, int64_t D, int64_t K, int64_t L, rq_codebook_ema_stats_form* form) {
  RQ_CHECK_ARG(form != nullptr, "rq_codebook_ema_stats_plan: null form");
  RQ_CHECK_ARG(ema_shape_ok(B, D, K, L),
               "rq_codebook_ema_stats: need 1 <= L <= 16, 1 <= K <= 4096, D %% 4 == 0, 4 <= D <= 1024, 0 <= B < 2^31 "
               "(B=%lld D=%lld K=%lld L=%lld)", (long long)B, (long long)D, (long long)K, (long long)L);
  const EmaPlan p = ema_plan(B, D, K);
  form->form = p.form;
  form->chunks = p.chunks;
  form->tiles = p.tiles;
  form->codes_per_tile = p.kt;
  form->rows_per_chunk = p.rows;
  form->lds_bytes = (int64_t)p.lds;
  return 0;
}

size_t rq_codebook_ema_stats_workspace(int64_t B, int64_t D, int64_t K, int64_t L) {
  if (!ema_shape_ok(B, D, K, L) || B == 0) return 0;
  const EmaPlan p = ema_plan(B, D, K);
  return (size_t)(L * p.chunks * K) * (size_t)(D + 1) * sizeof(float) + 16;
}

int rq_codebook_ema_stats(const float* res, const int64_t* ids, int64_t B, int64_t D, int64_t K, int64_t L, int64_t* n,
                          float* s, void* workspace, size_t ws_bytes, void* stream) {
  rq_codebook_ema_stats_form f;
  const int rc = rq_codebook_ema_stats_plan(B, D, K, L, &f);
  if (rc != 0) return rc;
  if (B == 0) return 0;
  RQ_CHECK_ARG(res && ids && n && s && workspace, "rq_codebook_ema_stats: null pointer");
  RQ_CHECK_ARG(((uintptr_t)res | (uintptr_t)s) % 16 == 0, "rq_codebook_ema_stats: res / s must be 16-byte aligned");
  RQ_CHECK_ARG(ws_bytes >= rq_codebook_ema_stats_workspace(B, D, K, L), "rq_codebook_ema_stats: workspace too small");
  float* part_s = reinterpret_cast<float*>(((uintptr_t)workspace + 15) & ~(uintptr_t)15);
  int* part_n = reinterpret_cast<int*>(part_s + L * f.chunks * K * D);
  hipLaunchKernelGGL(ema_stats_kernel, dim3((unsigned)f.chunks, (unsigned)L, (unsigned)f.tiles), dim3(64 * kEmaWaves),
                     (size_t)f.lds_bytes, (hipStream_t)stream, res, ids, B, (int)D, (int)K, (int)L, f.codes_per_tile,
                     f.rows_per_chunk, part_s, part_n);
  RQ_LAUNCH_CHECK("rq_codebook_ema_stats (chunks)");
  const int64_t KD = K * D;
  hipLaunchKernelGGL(ema_stats_reduce_kernel, dim3((unsigned)((KD / 4 + 255) / 256), (unsigned)L), dim3(256), 0,
                     (hipStream_t)stream, part_s, part_n, f.chunks, K, KD, s, n);
  RQ_LAUNCH_CHECK("rq_codebook_ema_stats (reduce)");
  return 0;
}

int rq_codebook_ema_apply(float* const* codebooks, int64_t L, int64_t K, int64_t D, float* N, float* S, int64_t* n,
                          float* s, double decay, double eps, void* stream) {
  RQ_CHECK_ARG(ema_shape_ok(0, D, K, L),
               "rq_codebook_ema_apply: need 1 <= L <= 16, 1 <= K <= 4096, D %% 4 == 0, 4 <= D <= 1024 (D=%lld K=%lld "
               "L=%lld)", (long long)D, (long long)K, (long long)L);
  RQ_CHECK_ARG(decay >= 0.0 && decay < 1.0 && eps > 0.0, "rq_codebook_ema_apply: need 0 <= decay < 1 and eps > 0");
  RQ_CHECK_ARG(codebooks && N && S && n && s, "rq_codebook_ema_apply: null pointer");
  RQ_CHECK_ARG(((uintptr_t)S | (uintptr_t)s) % 16 == 0, "rq_codebook_ema_apply: S / s must be 16-byte aligned");
  EmaTable tab;
  for (int l = 0; l < kReviveMaxL; ++l) {
    tab.cb[l] = l < L ? codebooks[l] : nullptr;
    if (l < L)
      RQ_CHECK_ARG(tab.cb[l] != nullptr && (uintptr_t)tab.cb[l] % 16 == 0,
                   "rq_codebook_ema_apply: codebook %d is null or not 16-byte aligned", l);
  }
  // decay and 1 - decay are each rounded to fp32 once, from the double (1.0f - (float)decay would carry the
  // rounding of decay at 1 / (1 - decay) times its relative size)
  hipLaunchKernelGGL(ema_apply_kernel, dim3((unsigned)L), dim3(kEmaApplyThreads), 0, (hipStream_t)stream, tab, (int)K,
                     (int)D, N, S, n, s, (float)decay, (float)(1.0 - decay), (float)eps, (float)((double)K * eps));
  RQ_LAUNCH_CHECK("rq_codebook_ema_apply");
  return 0;
}

}  // extern "C"
