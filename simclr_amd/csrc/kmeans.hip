// Spherical k-means probe (Lloyd's algorithm on L2-normalised bf16 features, R restarts trained in
// the same launches): the assignment step is a top-1 search over cosine similarities on
// v_mfma_f32_16x16x32_bf16, the centroid update a one-hot GEMM over the whole data set.  No
// [N][K] buffer exists at any point.  ops/kmeans.py holds the contract.
//
//   k_km_assign     block = 128 data rows; walks the [R · Kp][Fp] centroid matrix (all restarts,
//                   every restart padded to Kp = 16 · ceil(K / 16) rows) in tiles of 128 centroid
//                   rows, operands staged through LDS as in k_knn_topk.  The centroids are the
//                   MFMA's A operand and the data rows its B operand, so a lane's 4 accumulator
//                   elements are 4 centroids of one data row: the arg-max over a 16-centroid block
//                   is 3 in-lane compares and 2 cross-lane steps.  A 16-centroid block never spans
//                   two restarts (Kp is a multiple of 16).  The running (best, index) of every
//                   (row, restart) lives in LDS, owned by one lane of one wave (a wave owns 32 data
//                   rows and all 128 centroid rows of a tile), so there are no atomics on it and the
//                   order (sim descending, k ascending) makes the result independent of the walk.
//                   Writes a [R][N], s [R][N]; counts the rows per cluster (LDS histogram, integer
//                   atomics) and the rows whose assignment changed into changed[r][*it].
//   k_km_update     slab[split] = onehot(a)ᵀ · X over the split's rows: block = 128 centroid rows
//                   x 64 features, K-steps of 32 data rows in ascending order; the one-hot A
//                   operand is built in registers from the assignments (1.0 / 0.0 are exact in
//                   bf16), the X tile is transposed through LDS by xt_load / xt_store (common.h),
//                   as in the linear probes' k_linear_wgrad.
//   k_km_finish     block = one centroid row: merges the slabs in split order, norm in fp64,
//                   c = bf16(S / max(|S|, 1e-12)); a cluster without rows keeps its centroid bits.
//                   Clears the row's count for the next assign and advances the device-side
//                   iteration counter.
//   k_km_objective  J_r = Σ_i s[r][i] in fp64, fixed order (strided partial sums, then a tree).
//
// The number of splits depends on N and Fp only, so a restart's sums do not depend on R.
#include <algorithm>

#include "common.h"
#include "kernels.h"

namespace {

constexpr int KM_BM = 128, KM_BN = 128, KM_BK = 64, KM_KP = KM_BK + 8;
constexpr int KM_MAX_R = 16, KM_MAX_COLS = 1024;
constexpr int KM_NONE = 0x7fffffff;  // index of "no valid similarity seen"
constexpr int KM_UF = 64, KM_UM = 128, KM_UK = XT_ROWS, KM_UKP = XT_LD;
constexpr int KM_MAX_FP = 4096;

// (v, k) beats (bv, bk) under (sim descending, k ascending)
__device__ __forceinline__ bool km_better(float v, int k, float bv, int bk) {
  return v > bv || (v == bv && k < bk);
}

__global__ __launch_bounds__(256) void k_km_assign(const uint16_t* __restrict__ X,
                                                   const uint16_t* __restrict__ C, int N, int Fp,
                                                   int K, int Kp, int R, int* __restrict__ a,
                                                   float* __restrict__ s, int* __restrict__ counts,
                                                   int* __restrict__ changed,
                                                   const int* __restrict__ it, int Tp1) {
  // the operand tiles and the count histogram are never live at the same time
  __shared__ __attribute__((aligned(16))) uint16_t lds[2 * KM_BM * KM_KP];
  __shared__ float bestv[KM_MAX_R * KM_BM];  // [restart][row of the block]
  __shared__ int bestk[KM_MAX_R * KM_BM];
  __shared__ int chg[KM_MAX_R];
  static_assert(sizeof(int) * KM_MAX_COLS <= sizeof(uint16_t) * 2 * KM_BM * KM_KP, "histogram");
  uint16_t* Xs = lds;
  uint16_t* Cs = lds + KM_BM * KM_KP;
  int* hist = reinterpret_cast<int*>(lds);

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int li = lane & 15, g = lane >> 4;
  const int m0 = blockIdx.x * KM_BM;
  const int RK = R * Kp;

  for (int i = tid; i < KM_MAX_R * KM_BM; i += 256) { bestv[i] = -INFINITY; bestk[i] = KM_NONE; }
  if (tid < KM_MAX_R) chg[tid] = 0;

  // staging: 128 rows x 8 16-byte chunks per operand and K-step, 4 + 4 chunks per thread
  const int sr = tid >> 3, sc = tid & 7;  // rows sr + 32 p
  const uint16_t* xptr[4];
#pragma unroll
  for (int p = 0; p < 4; ++p) xptr[p] = X + (size_t)min(m0 + sr + 32 * p, N - 1) * Fp + sc * 8;

  for (int n0 = 0; n0 < RK; n0 += KM_BN) {
    __syncthreads();  // the operand tiles are free; the first pass: bestv / bestk are initialised
    const uint16_t* cptr[4];
#pragma unroll
    for (int p = 0; p < 4; ++p)
      cptr[p] = C + (size_t)min(n0 + sr + 32 * p, RK - 1) * Fp + sc * 8;

    f32x4 acc[8][2];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

    u32x4 rx[4], rc[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      rx[p] = *(const u32x4*)(xptr[p]);
      rc[p] = *(const u32x4*)(cptr[p]);
    }
    for (int kk = 0; kk < Fp; kk += KM_BK) {
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        *(u32x4*)(Xs + (sr + 32 * p) * KM_KP + sc * 8) = rx[p];
        *(u32x4*)(Cs + (sr + 32 * p) * KM_KP + sc * 8) = rc[p];
      }
      __syncthreads();
      if (kk + KM_BK < Fp) {
#pragma unroll
        for (int p = 0; p < 4; ++p) {
          rx[p] = *(const u32x4*)(xptr[p] + kk + KM_BK);
          rc[p] = *(const u32x4*)(cptr[p] + kk + KM_BK);
        }
      }
#pragma unroll
      for (int ks = 0; ks < KM_BK; ks += 32) {
        bf16x8 c[8], x[2];
#pragma unroll
        for (int i = 0; i < 8; ++i)
          c[i] = *(const bf16x8*)(Cs + (i * 16 + li) * KM_KP + ks + g * 8);
#pragma unroll
        for (int j = 0; j < 2; ++j)
          x[j] = *(const bf16x8*)(Xs + (wid * 32 + j * 16 + li) * KM_KP + ks + g * 8);
#pragma unroll
        for (int i = 0; i < 8; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(c[i], x[j], acc[i][j], 0, 0, 0);
      }
      __syncthreads();
    }

    // acc[i][j][r]: centroid row n0 + 16 i + 4 g + r, data row m0 + 32 wid + 16 j + li
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int cb = n0 + 16 * i;
      if (cb >= RK) continue;  // uniform
      const int r = cb / Kp;
      const int kb = cb - r * Kp + 4 * g;
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        float bv = -INFINITY;
        int bk = KM_NONE;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float v = acc[i][j][e] + 0.f;  // -0 -> +0: equal floats tie
          const int k = kb + e;
          // a padding column and a NaN never win; k ascends, so `>` keeps the lowest k of a tie
          if (k < K && v == v && (v > bv || bk == KM_NONE)) { bv = v; bk = k; }
        }
#pragma unroll
        for (int o = 16; o <= 32; o <<= 1) {
          const float ov = __shfl_xor(bv, o, 64);
          const int ok = __shfl_xor(bk, o, 64);
          if (km_better(ov, ok, bv, bk)) { bv = ov; bk = ok; }
        }
        if (g == 0) {
          const int o = r * KM_BM + wid * 32 + j * 16 + li;
          if (km_better(bv, bk, bestv[o], bestk[o])) { bestv[o] = bv; bestk[o] = bk; }
        }
      }
    }
  }

  __syncthreads();
  for (int i = tid; i < RK; i += 256) hist[i] = 0;
  __syncthreads();
  for (int i = tid; i < R * KM_BM; i += 256) {
    const int r = i / KM_BM, grow = m0 + (i % KM_BM);
    if (grow >= N) continue;
    int k = bestk[i];
    float v = bestv[i];
    if (k == KM_NONE) { k = 0; v = __uint_as_float(0x7fc00000u); }  // only NaN similarities
    const size_t o = (size_t)r * N + grow;
    const int old = a[o];
    a[o] = k;
    s[o] = v;
    atomicAdd(&hist[r * Kp + k], 1);
    if (old != k) atomicAdd(&chg[r], 1);
  }
  __syncthreads();
  for (int i = tid; i < RK; i += 256) {
    const int c = hist[i];
    if (c) atomicAdd(&counts[i], c);
  }
  const int t = *it;
  if (tid < R && chg[tid] && t >= 0 && t < Tp1) atomicAdd(&changed[(size_t)tid * Tp1 + t], chg[tid]);
}

// slab [splits][R · Kp][Fp] fp32.  grid (Fp / 64, ceil(R · Kp / 128), splits); split z owns the data
// rows [z · rps, (z + 1) · rps).
__global__ __launch_bounds__(256) void k_km_update(const uint16_t* __restrict__ X,
                                                   const int* __restrict__ a, int N, int Fp, int Kp,
                                                   int R, int rps, float* __restrict__ slab) {
  __shared__ __attribute__((aligned(16))) uint16_t Xs[KM_UF * KM_UKP];  // [feature][data row]
  __shared__ __attribute__((aligned(16))) int As[(KM_UM / 16) * KM_UK];  // [16-row block][data row]
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int li = lane & 15, g = lane >> 4;
  const int f0 = blockIdx.x * KM_UF, n0 = blockIdx.y * KM_UM;
  const int RK = R * Kp;
  const int ncnt = min(KM_UM / 16, (RK - n0) / 16);
  const int kbeg = min(N, (int)blockIdx.z * rps), kend = min(N, kbeg + rps);

  // staging: 32 data rows x 8 16-byte chunks of the feature tile, one chunk per thread (xt_load);
  // the assignments of the tile's (up to) 8 sixteen-centroid blocks, one value per thread
  const int aq = tid >> 5, ak = tid & 31;
  const int ar = aq < ncnt ? (n0 + 16 * aq) / Kp : 0;
  auto loadx = [&](int k0) -> u32x4 {
    return xt_load(k0, kend, tid, [&](int k) { return X + (size_t)k * Fp + f0; });
  };
  auto loada = [&](int k0) -> int {
    const int k = k0 + ak;
    return (aq < ncnt && k < kend) ? a[(size_t)ar * N + k] : -1;
  };
  int kid[KM_UM / 16];  // this lane's cluster within its restart, per 16-row block
#pragma unroll
  for (int i = 0; i < KM_UM / 16; ++i) {
    const int m = n0 + 16 * i + li;
    kid[i] = i < ncnt ? m - (m / Kp) * Kp : -2;
  }

  f32x4 acc[KM_UM / 16];
#pragma unroll
  for (int i = 0; i < KM_UM / 16; ++i) acc[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
  u32x4 rx = loadx(kbeg);
  int ra = loada(kbeg);
  for (int k0 = kbeg; k0 < kend; k0 += KM_UK) {
    xt_store(Xs, tid, rx);
    As[tid] = ra;
    __syncthreads();
    if (k0 + KM_UK < kend) {
      rx = loadx(k0 + KM_UK);
      ra = loada(k0 + KM_UK);
    }
    const bf16x8 b = *(const bf16x8*)(Xs + (16 * wid + li) * KM_UKP + g * 8);
#pragma unroll
    for (int i = 0; i < KM_UM / 16; ++i) {
      if (i < ncnt) {
        const int* ap = As + i * KM_UK + g * 8;
        const int4 a0 = *(const int4*)ap, a1 = *(const int4*)(ap + 4);
        const int kc = kid[i];
        u32x4 w;  // bf16 1.0 = 0x3f80
        w[0] = (a0.x == kc ? 0x3f80u : 0u) | (a0.y == kc ? 0x3f800000u : 0u);
        w[1] = (a0.z == kc ? 0x3f80u : 0u) | (a0.w == kc ? 0x3f800000u : 0u);
        w[2] = (a1.x == kc ? 0x3f80u : 0u) | (a1.y == kc ? 0x3f800000u : 0u);
        w[3] = (a1.z == kc ? 0x3f80u : 0u) | (a1.w == kc ? 0x3f800000u : 0u);
        acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, w), b, acc[i],
                                                         0, 0, 0);
      }
    }
    __syncthreads();
  }

  // acc[i][r]: centroid row n0 + 16 i + 4 g + r, feature f0 + 16 wid + li
  const int f = f0 + 16 * wid + li;
#pragma unroll
  for (int i = 0; i < KM_UM / 16; ++i) {
    if (i >= ncnt) continue;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int n = n0 + 16 * i + 4 * g + r;
      slab[((size_t)blockIdx.z * RK + n) * Fp + f] = acc[i][r];
    }
  }
}

// fixed-order block sum of one double per thread (256 threads); every thread gets the total
__device__ __forceinline__ double km_block_sum(double v, double* red, int tid) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  if ((tid & 63) == 0) red[tid >> 6] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

__global__ __launch_bounds__(256) void k_km_finish(const float* __restrict__ slab, int splits,
                                                   int RK, int Fp, int K, int Kp,
                                                   int* __restrict__ counts,
                                                   uint16_t* __restrict__ C, float* __restrict__ S,
                                                   int* __restrict__ it) {
  __shared__ double red[4];
  const int m = blockIdx.x, tid = threadIdx.x;
  if (m == 0 && tid == 0) *it += 1;
  if (m - (m / Kp) * Kp >= K) return;  // padding row: stays zero
  const int n = counts[m];
  __syncthreads();
  if (tid == 0) counts[m] = 0;  // consumed: the next assign counts from zero
  float sv[KM_MAX_FP / 256];
  double ss = 0.0;
#pragma unroll
  for (int q = 0; q < KM_MAX_FP / 256; ++q) {
    const int f = tid + 256 * q;
    sv[q] = 0.f;
    if (f < Fp) {
      float t = 0.f;
      for (int sp = 0; sp < splits; ++sp) t += slab[((size_t)sp * RK + m) * Fp + f];
      sv[q] = t;
      ss += (double)t * (double)t;
      if (S) S[(size_t)m * Fp + f] = t;
    }
  }
  ss = km_block_sum(ss, red, tid);
  if (n <= 0) return;  // an empty cluster keeps its centroid bit for bit
  const float den = fmaxf((float)sqrt(ss), 1e-12f);
#pragma unroll
  for (int q = 0; q < KM_MAX_FP / 256; ++q) {
    const int f = tid + 256 * q;
    if (f < Fp) C[(size_t)m * Fp + f] = f2bf(sv[q] / den);
  }
}

__global__ __launch_bounds__(256) void k_km_objective(const float* __restrict__ s, int N,
                                                      double* __restrict__ J) {
  __shared__ double red[4];
  const int r = blockIdx.x, tid = threadIdx.x;
  double acc = 0.0;
  for (int i = tid; i < N; i += 256) acc += (double)s[(size_t)r * N + i];
  acc = km_block_sum(acc, red, tid);
  if (tid == 0) J[r] = acc;
}

}  // namespace

int km_kstep() { return KM_BK; }
int km_max_restarts() { return KM_MAX_R; }
int km_max_cols() { return KM_MAX_COLS; }
int km_max_fp() { return KM_MAX_FP; }

// Row splits of the update: about 1024 rows each, fewer for wide features (the slabs are
// splits · R · Kp · Fp floats).  A function of N and Fp only: a restart's sums must not depend on R.
int km_splits(int N, int Fp) {
  const int cap = std::min(32, std::max(4, 16384 / std::max(Fp, 1)));
  return std::max(1, std::min(cap, (N + 1023) / 1024));
}

size_t km_slab_floats(int N, int Fp, int RK) { return (size_t)km_splits(N, Fp) * RK * Fp; }

void km_assign(const uint16_t* X, const uint16_t* C, int N, int Fp, int K, int Kp, int R, int* a,
               float* s, int* counts, int* changed, const int* it, int Tp1, hipStream_t st) {
  hipLaunchKernelGGL(k_km_assign, dim3((N + KM_BM - 1) / KM_BM), dim3(256), 0, st, X, C, N, Fp, K,
                     Kp, R, a, s, counts, changed, it, Tp1);
  HIP_CHECK_LAUNCH();
}

void km_update(const uint16_t* X, const int* a, int N, int Fp, int K, int Kp, int R, int* counts,
               uint16_t* C, float* S, float* slab, int* it, hipStream_t st) {
  const int RK = R * Kp, splits = km_splits(N, Fp);
  const int rps = ((N + splits - 1) / splits + KM_UK - 1) / KM_UK * KM_UK;
  hipLaunchKernelGGL(k_km_update, dim3(Fp / KM_UF, (RK + KM_UM - 1) / KM_UM, splits), dim3(256), 0,
                     st, X, a, N, Fp, Kp, R, rps, slab);
  HIP_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_km_finish, dim3(RK), dim3(256), 0, st, slab, splits, RK, Fp, K, Kp, counts,
                     C, S, it);
  HIP_CHECK_LAUNCH();
}

void km_objective(const float* s, int R, int N, double* J, hipStream_t st) {
  hipLaunchKernelGGL(k_km_objective, dim3(R), dim3(256), 0, st, s, N, J);
  HIP_CHECK_LAUNCH();
}
