// Codebook usage counters and dead-code revival for the RQ-VAE tokenizer.
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

}  // extern "C"
