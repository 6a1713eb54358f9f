// Weighted k-nearest-neighbour probe (Wu et al., InstDisc; the training-free probe of the
// SimCLR / MoCo family): cosine similarities of every query against a feature bank on
// v_mfma_f32_16x16x32_bf16, consumed in registers by an exact top-k selection, and the
// temperature-weighted class vote over the selected neighbours.  No [Q][N] buffer exists at any
// point; scratch is O(Q · capacity · splits).
//
//   k_knn_normalize   rows L2-normalised in fp32 (F.normalize: x / max(|x|, 1e-12), the norm
//                     accumulated in fp64 and rounded to fp32), rounded once to bf16, columns padded with zeros to the K-step.  One wave per row.
//   k_knn_topk        block (query tile of 128 rows, bank split): 128x128 similarity tiles from
//                     LDS-staged operands (fragment layout and LDS padding of k_gemm_sk).  Every
//                     query row keeps a threshold tau (its current k-th best, -inf until k
//                     candidates were seen) and an append buffer of KNN_CAP (sim, index) keys in
//                     global memory that only this block touches.  The tile epilogue appends the
//                     in-range, non-self elements above tau (a NaN compares false and is never
//                     appended).  Before a tile that could overflow a buffer (count + 128 >
//                     KNN_CAP) the block compacts: one wave per row sorts the row's keys in LDS
//                     (bitonic), keeps k and sets tau to the k-th.  A tile appends at most 128 keys
//                     to a row and a compacted row holds at most k <= 256, so a buffer never
//                     overflows by construction; the append is bounds-checked regardless.
//   k_knn_merge       per query row: the splits' candidates sorted once more, the first k written
//                     as vals / idx (unfilled slots: -inf / -1).
//   k_knn_vote        per query row: score[c] = Σ_{j: label_j = c} exp((sim_j - 1) / T) in the
//                     neighbours' sorted order (lane c % 64 owns class c), and the target's rank.
//
// A key is (~orderable(sim) << 32) | index, so ascending unsigned order is (sim descending,
// index ascending): a total order, hence bitwise repeatable results whatever order the appends
// landed in.  A split walks its bank columns in ascending order, so a later element that ties the
// k-th similarity always has a larger index and `sim > tau` is exact.
#include <algorithm>

#include "common.h"
#include "kernels.h"

namespace {

constexpr int KNN_BM = 128, KNN_BN = 128, KNN_BK = 64, KNN_KP = KNN_BK + 8;
constexpr int KNN_CAP = 512;         // keys per row buffer: >= max k (256) + KNN_BN
constexpr int KNN_MAX_K = 256, KNN_MAX_SPLITS = 8, KNN_MAX_C = 1024;
constexpr int KNN_MERGE_CAP = KNN_MAX_K * KNN_MAX_SPLITS;
constexpr unsigned long long KNN_EMPTY = ~0ull;
typedef unsigned long long knn_key;

__device__ __forceinline__ knn_key knn_make_key(float v, int idx) {
  const uint32_t b = __float_as_uint(v);
  const uint32_t o = b ^ ((b >> 31) ? 0xffffffffu : 0x80000000u);  // ascending with v
  return ((knn_key)(~o) << 32) | (uint32_t)idx;
}

__device__ __forceinline__ float knn_key_val(knn_key key) {
  const uint32_t o = ~(uint32_t)(key >> 32);
  return __uint_as_float((o & 0x80000000u) ? (o ^ 0x80000000u) : ~o);
}

// Ascending bitonic sort of s[0, P) by one wave, P a power of two.  LDS operations of one wave
// complete in issue order, so the stages need no block barrier.
__device__ __forceinline__ void knn_wave_sort(knn_key* s, int P, int lane) {
  for (int size = 2; size <= P; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int i = lane; i < (P >> 1); i += 64) {
        const int lo = ((i & ~(stride - 1)) << 1) | (i & (stride - 1));
        const int hi = lo + stride;
        const bool asc = (lo & size) == 0;
        const knn_key a = s[lo], b = s[hi];
        if ((a > b) == asc) { s[lo] = b; s[hi] = a; }
      }
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      __builtin_amdgcn_wave_barrier();
    }
  }
}

__device__ __forceinline__ int knn_pow2(int n) {
  int p = 2;
  while (p < n) p <<= 1;
  return p;
}

template <typename T> __device__ __forceinline__ float knn_ld(const T* p);
template <> __device__ __forceinline__ float knn_ld<float>(const float* p) { return *p; }
template <> __device__ __forceinline__ float knn_ld<uint16_t>(const uint16_t* p) { return bf2f(*p); }

template <typename T>
__global__ __launch_bounds__(256) void k_knn_normalize(const T* __restrict__ x, int R, int D,
                                                       int Dp, uint16_t* __restrict__ out) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= R) return;
  const T* src = x + (size_t)row * D;
  // the norm in fp64 (squares of fp32 values are exact there), rounded once to fp32: the result
  // does not depend on the summation order, so the torch path rounds to the same bf16 operands
  double ss = 0.0;
  for (int d = lane; d < D; d += 64) {
    const double v = (double)knn_ld(src + d);
    ss += v * v;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) ss += __shfl_xor(ss, o, 64);
  const float den = fmaxf((float)sqrt(ss), 1e-12f);  // F.normalize eps
  uint16_t* dst = out + (size_t)row * Dp;
  for (int d = lane; d < Dp; d += 64) dst[d] = d < D ? f2bf(knn_ld(src + d) / den) : (uint16_t)0;
}

// rows [0, KNN_BM) of this block with more than k keys: sort, keep the best k, set tau
__device__ __forceinline__ void knn_compact(knn_key* mybuf, knn_key* sortbuf,
                                            int* cnt, float* tau, int k, int wid, int lane) {
  knn_key* s = sortbuf + wid * KNN_CAP;
  for (int r = wid; r < KNN_BM; r += 4) {
    const int n = min(cnt[r], KNN_CAP);
    if (n <= k) continue;
    const int P = knn_pow2(n);
    knn_key* g = mybuf + (size_t)r * KNN_CAP;
    for (int i = lane; i < P; i += 64) s[i] = i < n ? g[i] : KNN_EMPTY;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    knn_wave_sort(s, P, lane);
    for (int i = lane; i < k; i += 64) g[i] = s[i];
    if (lane == 0) {
      cnt[r] = k;
      tau[r] = knn_key_val(s[k - 1]);
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
}

// Qn [Q][Dp], Bn [N][Dp] bf16 (normalised, zero-padded).  grid (query tiles, splits); split y
// owns the bank tiles [y · tps, (y + 1) · tps).  buf [blocks][KNN_BM][KNN_CAP] keys, private to
// the block; cand [Q][splits][k] keys (KNN_EMPTY where a split had fewer than k).
__global__ __launch_bounds__(256) void k_knn_topk(const uint16_t* __restrict__ Qn,
                                                  const uint16_t* __restrict__ Bn, int Q, int N,
                                                  int Dp, int k, int has_self, long long self_off,
                                                  int tps, knn_key* buf,
                                                  knn_key* __restrict__ cand) {
  // the operand tiles and the sort space are never live at the same time
  __shared__ __attribute__((aligned(16))) uint16_t lds[2 * KNN_BM * KNN_KP];
  __shared__ int cnt[KNN_BM];
  __shared__ float tau[KNN_BM];
  static_assert(sizeof(knn_key) * 4 * KNN_CAP <= sizeof(uint16_t) * 2 * KNN_BM * KNN_KP, "sort space");
  static_assert(KNN_CAP >= KNN_MAX_K + KNN_BN, "a compacted row must take one more tile");
  uint16_t* As = lds;
  uint16_t* Bs = lds + KNN_BM * KNN_KP;
  knn_key* sortbuf = reinterpret_cast<knn_key*>(lds);

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int li = lane & 15, g = lane >> 4;
  const int wm = (wid >> 1) * 64, wn = (wid & 1) * 64;
  const int m0 = blockIdx.x * KNN_BM;
  const int ntiles = (N + KNN_BN - 1) / KNN_BN;
  const int t0 = blockIdx.y * tps, t1 = min(ntiles, t0 + tps);
  knn_key* mybuf = buf + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * KNN_BM * KNN_CAP;

  if (tid < KNN_BM) { cnt[tid] = 0; tau[tid] = -INFINITY; }

  // staging: 128 rows x 8 16-byte chunks per operand and K-step, 4 + 4 chunks per thread
  const int sr = tid >> 3, sc = tid & 7;  // rows sr + 32 p
  const uint16_t* aptr[4];
#pragma unroll
  for (int p = 0; p < 4; ++p)
    aptr[p] = Qn + (size_t)min(m0 + sr + 32 * p, Q - 1) * Dp + sc * 8;

  for (int t = t0; t < t1; ++t) {
    const int n0 = t * KNN_BN;
    __syncthreads();  // the appends of the previous tile are visible; the operand tiles are free
    const int need = (tid < KNN_BM) ? (cnt[tid] + KNN_BN > KNN_CAP) : 0;
    if (__syncthreads_or(need)) {
      knn_compact(mybuf, sortbuf, cnt, tau, k, wid, lane);
      __syncthreads();
    }
    const uint16_t* bptr[4];
#pragma unroll
    for (int p = 0; p < 4; ++p)
      bptr[p] = Bn + (size_t)min(n0 + sr + 32 * p, N - 1) * Dp + sc * 8;

    f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

    u32x4 ra[4], rb[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      ra[p] = *(const u32x4*)(aptr[p]);
      rb[p] = *(const u32x4*)(bptr[p]);
    }
    for (int kk = 0; kk < Dp; kk += KNN_BK) {
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        *(u32x4*)(As + (sr + 32 * p) * KNN_KP + sc * 8) = ra[p];
        *(u32x4*)(Bs + (sr + 32 * p) * KNN_KP + sc * 8) = rb[p];
      }
      __syncthreads();
      if (kk + KNN_BK < Dp) {
#pragma unroll
        for (int p = 0; p < 4; ++p) {
          ra[p] = *(const u32x4*)(aptr[p] + kk + KNN_BK);
          rb[p] = *(const u32x4*)(bptr[p] + kk + KNN_BK);
        }
      }
#pragma unroll
      for (int ks = 0; ks < KNN_BK; ks += 32) {
        bf16x8 a[4], b[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          a[i] = *(const bf16x8*)(As + (wm + i * 16 + li) * KNN_KP + ks + g * 8);
          b[i] = *(const bf16x8*)(Bs + (wn + i * 16 + li) * KNN_KP + ks + g * 8);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[i], b[j], acc[i][j], 0, 0, 0);
      }
      __syncthreads();
    }

    // acc[i][j][r]: query row wm + 16 i + 4 g + r, bank column wn + 16 j + li
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = wm + i * 16 + 4 * g + r;
        const int grow = m0 + row;
        if (grow >= Q) continue;
        const float th = tau[row];
        const long long self_col = has_self ? self_off + grow : -1;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int col = n0 + wn + j * 16 + li;
          const float v = acc[i][j][r] + 0.f;  // -0 -> +0: equal floats get equal keys
          if (col < N && v > th && (long long)col != self_col) {
            const int pos = atomicAdd(&cnt[row], 1);
            if (pos < KNN_CAP) mybuf[(size_t)row * KNN_CAP + pos] = knn_make_key(v, col);
          }
        }
      }
    }
  }

  __syncthreads();
  knn_compact(mybuf, sortbuf, cnt, tau, k, wid, lane);
  __syncthreads();
  const int splits = gridDim.y;
  for (int r = wid; r < KNN_BM; r += 4) {
    const int grow = m0 + r;
    if (grow >= Q) break;
    const int n = min(cnt[r], k);
    knn_key* dst = cand + ((size_t)grow * splits + blockIdx.y) * k;
    const knn_key* src = mybuf + (size_t)r * KNN_CAP;
    for (int i = lane; i < k; i += 64) dst[i] = i < n ? src[i] : KNN_EMPTY;
  }
}

// one wave per query row: sort the splits' candidates, write the first k
__global__ __launch_bounds__(64) void k_knn_merge(const knn_key* __restrict__ cand, int Q,
                                                  int splits, int k, float* __restrict__ vals,
                                                  int* __restrict__ idx) {
  __shared__ knn_key s[KNN_MERGE_CAP];
  const int row = blockIdx.x, lane = threadIdx.x;
  if (row >= Q) return;
  const int total = min(splits * k, KNN_MERGE_CAP);
  const int P = knn_pow2(total);
  const knn_key* src = cand + (size_t)row * splits * k;
  for (int i = lane; i < P; i += 64) s[i] = i < total ? src[i] : KNN_EMPTY;
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
  knn_wave_sort(s, P, lane);
  for (int i = lane; i < k; i += 64) {
    const knn_key key = s[i];
    const bool ok = key != KNN_EMPTY;
    vals[(size_t)row * k + i] = ok ? knn_key_val(key) : -INFINITY;
    idx[(size_t)row * k + i] = ok ? (int)(uint32_t)key : -1;
  }
}

// vals / idx [Q][k] sorted, labels [N], targets [Q] -> scores [Q][C], rank [Q].  One wave per
// query; lane c % 64 owns class c and walks the neighbours in order, so a class's sum has a fixed
// order.  rank = #{c: score[c] > score[t]} + #{c < t: score[c] == score[t]}; a target class
// without a neighbour (or out of range) gets rank C.
__global__ __launch_bounds__(256) void k_knn_vote(const float* __restrict__ vals,
                                                  const int* __restrict__ idx,
                                                  const int64_t* __restrict__ labels,
                                                  const int64_t* __restrict__ targets, int Q, int k,
                                                  int N, int C, float inv_t,
                                                  float* __restrict__ scores,
                                                  int* __restrict__ rank) {
  __shared__ float sc_all[4][KNN_MAX_C];
  __shared__ float w_all[4][KNN_MAX_K];
  __shared__ int lab_all[4][KNN_MAX_K];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int row = blockIdx.x * 4 + wid;
  if (row >= Q) return;
  float* sc = sc_all[wid];
  float* w = w_all[wid];
  int* lab = lab_all[wid];
  for (int c = lane; c < C; c += 64) sc[c] = 0.f;
  for (int j = lane; j < k; j += 64) {
    const int b = idx[(size_t)row * k + j];
    int l = -1;
    if (b >= 0 && b < N) {
      const int64_t l64 = labels[b];
      if (l64 >= 0 && l64 < C) l = (int)l64;
    }
    lab[j] = l;
    w[j] = l >= 0 ? expf((vals[(size_t)row * k + j] - 1.f) * inv_t) : 0.f;
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
  const int64_t t64 = targets[row];
  const int t = (t64 >= 0 && t64 < C) ? (int)t64 : -1;
  int hit = 0;
  for (int j = 0; j < k; ++j) {
    const int l = lab[j];
    if (l >= 0 && (l & 63) == lane) {
      sc[l] += w[j];
      hit |= (l == t);
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
  hit = __any(hit);
  const float st = t >= 0 ? sc[t] : 0.f;
  int above = 0;
  for (int c = lane; c < C; c += 64) {
    const float v = sc[c];
    scores[(size_t)row * C + c] = v;
    above += (v > st || (v == st && c < t)) ? 1 : 0;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) above += __shfl_xor(above, o, 64);
  if (lane == 0) rank[row] = (t >= 0 && hit) ? above : C;
}

}  // namespace

int knn_kstep() { return KNN_BK; }
int knn_max_k() { return KNN_MAX_K; }
int knn_max_classes() { return KNN_MAX_C; }

size_t knn_topk_lds() {
  return sizeof(uint16_t) * 2 * KNN_BM * KNN_KP + KNN_BM * (sizeof(int) + sizeof(float));
}

// Bank splits: enough blocks for two waves of the 256 CUs, at least 8 bank tiles per split.
int knn_splits(int Q, int N) {
  const int qt = (Q + KNN_BM - 1) / KNN_BM, nt = (N + KNN_BN - 1) / KNN_BN;
  int s = (512 + qt - 1) / qt;
  s = std::min(s, std::min(KNN_MAX_SPLITS, std::max(1, nt / 8)));
  s = std::max(s, 1);
  const int tps = (nt + s - 1) / s;
  return (nt + tps - 1) / tps;  // no empty split
}

size_t knn_buf_keys(int Q, int N) {
  const size_t qt = (Q + KNN_BM - 1) / KNN_BM;
  return qt * knn_splits(Q, N) * KNN_BM * KNN_CAP;
}

size_t knn_cand_keys(int Q, int N, int k) { return (size_t)Q * knn_splits(Q, N) * k; }

void knn_normalize(const void* x, bool x_is_bf16, int R, int D, int Dp, uint16_t* out,
                   hipStream_t s) {
  const dim3 grid((R + 3) / 4);
  if (x_is_bf16)
    hipLaunchKernelGGL(k_knn_normalize<uint16_t>, grid, dim3(256), 0, s, (const uint16_t*)x, R, D,
                       Dp, out);
  else
    hipLaunchKernelGGL(k_knn_normalize<float>, grid, dim3(256), 0, s, (const float*)x, R, D, Dp,
                       out);
  HIP_CHECK_LAUNCH();
}

void knn_topk(const uint16_t* Qn, const uint16_t* Bn, int Q, int N, int Dp, int k, bool has_self,
              long long self_off, unsigned long long* buf, unsigned long long* cand, float* vals,
              int* idx, hipStream_t s) {
  const int qt = (Q + KNN_BM - 1) / KNN_BM, nt = (N + KNN_BN - 1) / KNN_BN;
  const int splits = knn_splits(Q, N);
  const int tps = (nt + splits - 1) / splits;
  hipLaunchKernelGGL(k_knn_topk, dim3(qt, splits), dim3(256), 0, s, Qn, Bn, Q, N, Dp, k,
                     has_self ? 1 : 0, self_off, tps, buf, cand);
  HIP_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_knn_merge, dim3(Q), dim3(64), 0, s, cand, Q, splits, k, vals, idx);
  HIP_CHECK_LAUNCH();
}

void knn_vote(const float* vals, const int* idx, const int64_t* labels, const int64_t* targets,
              int Q, int k, int N, int C, float inv_t, float* scores, int* rank, hipStream_t s) {
  hipLaunchKernelGGL(k_knn_vote, dim3((Q + 3) / 4), dim3(256), 0, s, vals, idx, labels, targets, Q,
                     k, N, C, inv_t, scores, rank);
  HIP_CHECK_LAUNCH();
}
