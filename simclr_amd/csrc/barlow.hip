// Barlow Twins loss (Zbontar et al., 2021) on gfx950: per-view batch standardisation, the D x D
// cross-correlation of the two views on v_mfma_f32_16x16x32_bf16 (the contraction runs over the
// BATCH, K = n), the loss on it, and the whole backward.  Contract: loss/barlow.py.
//
//   forward   k_bt_standardize  z [2n][D] -> rstd [2][D], ẑ bf16 [2n][D], ẑT bf16 [2][D][n]
//             k_bt_corr         partial slabs [splits][D][D] = ẑ0T · ẑ1Tᵀ over a slice of the batch
//             k_bt_loss         C = (Σ_s slab_s) / n in split order, per-block loss partials
//             (+ ntxent_reduce_loss over the partials)
//   backward  k_bt_grad         G, Gᵀ bf16 from C and the upstream scalar g
//             k_bt_bwd          dẑ_v = ẑ_other · G(ᵀ) / n (K = D), per-tile column sums of dẑ and dẑ·ẑ
//             k_bt_std_bwd      dz = rstd · (dẑ − mean_b dẑ − ẑ · mean_b(dẑ·ẑ))
//   over all ranks (loss.barlow_global), around three collectives:
//             k_bt_stats, k_bt_merge_standardize  for k_bt_standardize: the same row passes
//               (bt_row_stats) and the same write pass (bt_write_zhat), the rank merge between
//             k_bt_slab_merge   Σ_s slab_s alone (bt_slab_sum, as k_bt_loss), for the all-reduce
//             k_bt_colsum       the tile sums alone (bt_part_sum, as k_bt_std_bwd), for the
//               all-gather; k_bt_std_bwd then adds the ranks' sums instead of the tiles'
//
// No atomics; every sum has a fixed order (rows by row group, splits and tiles by index), so the
// results are the same bits every run.  n % 32 == 0, D % 64 == 0, 64 <= D <= 2048 (the bindings
// check them before any launch).  The MFMA operands are read straight from global memory (the
// whole problem is L2-resident): lane (li = lane & 15, g = lane >> 4) holds row li, k = 8g..8g+7
// of its operand, and acc[r] is (A row 4g + r, B row li), as in k_gemm_sk.
#include "common.h"
#include "kernels.h"

namespace {

__device__ __forceinline__ float ldz(const uint16_t* p) { return bf2f(*p); }
__device__ __forceinline__ float ldz(const float* p) { return *p; }

// correctly rounded fp32 quotient and square root whatever the compile flags: evaluated in fp64
// (53 bits make the second rounding innocuous), so the statistics have the bits of an IEEE host.
// The empty asm keeps the compiler from narrowing (float)f((double)x) back to the fp32
// operation, whose default lowering here is not correctly rounded.
__device__ __forceinline__ double opaque(double x) {
  asm volatile("" : "+v"(x));
  return x;
}
__device__ __forceinline__ float div_rn(float a, float b) {
  return (float)opaque(opaque((double)a) / opaque((double)b));
}
__device__ __forceinline__ float sqrt_rn(float a) { return (float)opaque(sqrt(opaque((double)a))); }

constexpr int BT_RG = 16;  // row groups of the standardisation block (1024 threads)

// The two row passes of a (D/64, 2 views) x 1024-thread block: column tx of 64, row group ty of
// 16; zv = the view's column.  Mean, then centred sum of squares; group ty sums rows ty, ty + 16,
// ... in order, then the groups are summed in order — the order loss/barlow.py's twin uses, and
// the mean is correctly rounded, so the statistics have the bits of the twin on an IEEE host.
// Returns μ in every thread; m2 = Σ_b (z − μ)² (not divided) in the ty == 0 threads only.
template <typename T>
__device__ __forceinline__ float bt_row_stats(const T* zv, int n, int D, float& m2) {
#pragma clang fp contract(off)  // (c · c and the sum round separately, as the twin's do)
  __shared__ float red[BT_RG][64];
  __shared__ float s_mu[64];
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  float s = 0.f;
  for (int b = ty; b < n; b += BT_RG) s += ldz(zv + (size_t)b * D);
  red[ty][tx] = s;
  __syncthreads();
  if (ty == 0) {
    float t = 0.f;
    for (int k = 0; k < BT_RG; ++k) t += red[k][tx];
    s_mu[tx] = div_rn(t, (float)n);
  }
  __syncthreads();
  const float mu = s_mu[tx];
  s = 0.f;
  for (int b = ty; b < n; b += BT_RG) {
    const float c = ldz(zv + (size_t)b * D) - mu;
    s += c * c;
  }
  red[ty][tx] = s;
  __syncthreads();
  if (ty == 0) {
    float t = 0.f;
    for (int k = 0; k < BT_RG; ++k) t += red[k][tx];
    m2 = t;
  }
  return mu;
}

// rstd = 1 / sqrt(m2 / rows + eps), every step correctly rounded
__device__ __forceinline__ float bt_rstd(float m2, float rows, float eps) {
  return div_rn(1.f, sqrt_rn(div_rn(m2, rows) + eps));
}

// The write pass of the same block: ẑ = (z − μ) · rstd rounded once to bf16, for the view's n
// rows in chunks of 32, and through an LDS tile its transpose.  A thread's two rows of a chunk are
// written out and go to the tile as one 32-bit write: inside a helper the compiler no longer
// pairs them by itself (profiles/barlow_unify.md).
template <typename T>
__device__ __forceinline__ void bt_write_zhat(const T* zv, int v, int d0, int n, int D, float mu,
                                              float rs, uint16_t* __restrict__ zh,
                                              uint16_t* __restrict__ zhT) {
  __shared__ __align__(4) uint16_t tile[64][34];  // [column][row of the 32-row chunk]
  const int tx = threadIdx.x & 63, r = (threadIdx.x >> 6) * 2;  // this thread's rows: r, r + 1
  const int rl = threadIdx.x & 31, tc = threadIdx.x >> 5;  // the transposed write's row, column
  for (int r0 = 0; r0 < n; r0 += 32) {
    const float x0 = ldz(zv + (size_t)(r0 + r) * D), x1 = ldz(zv + (size_t)(r0 + r + 1) * D);
    const uint16_t h0 = f2bf((x0 - mu) * rs), h1 = f2bf((x1 - mu) * rs);
    zh[(size_t)(v * n + r0 + r) * D + d0 + tx] = h0;
    zh[(size_t)(v * n + r0 + r + 1) * D + d0 + tx] = h1;
    *(uint32_t*)&tile[tx][r] = (uint32_t)h0 | ((uint32_t)h1 << 16);  // (row stride 68 B, r even)
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int c = tc + 32 * k;
      zhT[((size_t)v * D + d0 + c) * n + r0 + rl] = tile[c][rl];
    }
    __syncthreads();
  }
}

// grid (D/64, 2 views), 1024 threads: the row passes, rstd, the write pass
template <typename T>
__global__ __launch_bounds__(1024) void k_bt_standardize(const T* __restrict__ z, int n, int D,
                                                         float eps, float* __restrict__ rstd,
                                                         uint16_t* __restrict__ zh,
                                                         uint16_t* __restrict__ zhT) {
  __shared__ float s_rs[64];
  const int v = blockIdx.y, d0 = blockIdx.x * 64;
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const T* zv = z + (size_t)v * n * D + d0 + tx;
  float m2 = 0.f;  // (set by the ty == 0 threads, read by them alone)
  const float mu = bt_row_stats(zv, n, D, m2);
  if (ty == 0) {
    const float rs = bt_rstd(m2, (float)n, eps);
    s_rs[tx] = rs;
    rstd[(size_t)v * D + d0 + tx] = rs;
  }
  __syncthreads();
  bt_write_zhat(zv, v, d0, n, D, mu, s_rs[tx], zh, zhT);
}

// Σ_{s < splits} slab_s in split order, four consecutive entries (float4 i4 of the D²/4) per thread
__device__ __forceinline__ float4 bt_slab_sum(const float* part, int splits, int D, size_t i4) {
  const size_t n4 = (size_t)D * D / 4;
  const float4* p = (const float4*)part;
  float4 a = p[i4];
  for (int s = 1; s < splits; ++s) {
    const float4 x = p[(size_t)s * n4 + i4];
    a.x += x.x; a.y += x.y; a.z += x.z; a.w += x.w;
  }
  return a;
}

// Σ_{p < parts} src[p · stride] in ascending order from 0.f: the row tiles' (or the ranks') column
// sums of dẑ and dẑ·ẑ
__device__ __forceinline__ float bt_part_sum(const float* src, int parts, size_t stride) {
  float s = 0.f;
  for (int p = 0; p < parts; ++p) s += src[p * stride];
  return s;
}

// grid (D/64, D/64, splits), 4 waves of 32 x 32: slab[z][i][j] = Σ_{b in the slice} ẑ0T[i][b] ẑ1T[j][b]
__global__ __launch_bounds__(256) void k_bt_corr(const uint16_t* __restrict__ zhT, int n, int D,
                                                 int kslice, float* __restrict__ part) {
  const uint16_t* A = zhT;
  const uint16_t* B = zhT + (size_t)D * n;
  const int m0 = blockIdx.x * 64, n0 = blockIdx.y * 64;
  const int k_beg = blockIdx.z * kslice;
  int k_end = k_beg + kslice;
  if (k_end > n) k_end = n;
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int li = lane & 15, g = lane >> 4;
  const int wm = (wid >> 1) * 32, wn = (wid & 1) * 32;
  const uint16_t* ap[2];
  const uint16_t* bp[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    ap[i] = A + (size_t)(m0 + wm + i * 16 + li) * n + g * 8;
    bp[i] = B + (size_t)(n0 + wn + i * 16 + li) * n + g * 8;
  }
  f32x4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
  for (int k = k_beg; k < k_end; k += 32) {
    bf16x8 a[2], b[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      a[i] = *(const bf16x8*)(ap[i] + k);
      b[i] = *(const bf16x8*)(bp[i] + k);
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[i], b[j], acc[i][j], 0, 0, 0);
  }
  float* out = part + (size_t)blockIdx.z * D * D;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        out[(size_t)(m0 + wm + i * 16 + 4 * g + r) * D + n0 + wn + j * 16 + li] = acc[i][j][r];
}

// four consecutive entries of one row per thread (D²/4 is a multiple of the 256-thread block):
// C = (Σ_s slab_s) / n, term = (1 − C_ii)² on the diagonal, (λ C_ij) C_ij off it;
// lpart[block] = the block's terms, lanes by wave_sum, waves in order
__global__ __launch_bounds__(256) void k_bt_loss(const float* __restrict__ part, int splits, int n,
                                                 int D, float lambd, float* __restrict__ C,
                                                 float* __restrict__ lpart) {
  __shared__ float red[4];
  const size_t i4 = (size_t)blockIdx.x * 256 + threadIdx.x;
  float4 a = bt_slab_sum(part, splits, D, i4);
  const float fn = (float)n;
  a.x /= fn; a.y /= fn; a.z /= fn; a.w /= fn;
  ((float4*)C)[i4] = a;
  const int row = (int)(i4 * 4 / D), col = (int)(i4 * 4 % D);
  const float c[4] = {a.x, a.y, a.z, a.w};
  float t = 0.f;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const float om = 1.f - c[e];
    t += (col + e == row) ? om * om : (lambd * c[e]) * c[e];
  }
  t = wave_sum(t);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = t;
  __syncthreads();
  if (threadIdx.x == 0) lpart[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

// grid (D/64, D/64): G_ii = −2g(1 − C_ii), G_ij = (2gλ) C_ij, rounded to bf16 once; G row-major
// and, through an LDS tile, Gᵀ
__global__ __launch_bounds__(256) void k_bt_grad(const float* __restrict__ C, int D, float lambd,
                                                 const float* __restrict__ gout,
                                                 uint16_t* __restrict__ G,
                                                 uint16_t* __restrict__ GT) {
  __shared__ uint16_t tile[64][66];
  const int i0 = blockIdx.y * 64, j0 = blockIdx.x * 64;
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const float g = gout[0];
  const float gd = -2.f * g, go = 2.f * g * lambd;
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    const int r = ty * 16 + k;
    const int i = i0 + r, j = j0 + tx;
    const float c = C[(size_t)i * D + j];
    const uint16_t h = f2bf(i == j ? gd * (1.f - c) : go * c);
    G[(size_t)i * D + j] = h;
    tile[r][tx] = h;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    const int r = ty * 16 + k;  // column j0 + r of G = row of Gᵀ
    GT[(size_t)(j0 + r) * D + i0 + tx] = tile[tx][r];
  }
}

// grid (n/32, D/64, 2 views), 4 waves of 16 x 32: dẑ_v[b][c] = Σ_k ẑ_other[b][k] Gv[c][k] / n with
// G0 = G, G1 = Gᵀ; colpart[v][row tile][0][c] = Σ_{32 rows} dẑ, [1][c] = Σ dẑ·ẑ_v
__global__ __launch_bounds__(256) void k_bt_bwd(const uint16_t* __restrict__ zh,
                                                const uint16_t* __restrict__ G,
                                                const uint16_t* __restrict__ GT, int n, int D,
                                                float* __restrict__ dzh,
                                                float* __restrict__ colpart) {
  __shared__ float red[2][2][64];  // [row half][dẑ | dẑ·ẑ][column]
  const int v = blockIdx.z;
  const uint16_t* A = zh + (size_t)(1 - v) * n * D;
  const uint16_t* B = v == 0 ? G : GT;
  const uint16_t* own = zh + (size_t)v * n * D;
  const int m0 = blockIdx.x * 32, c0 = blockIdx.y * 64;
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int li = lane & 15, g = lane >> 4;
  const int wm = (wid >> 1) * 16, wn = (wid & 1) * 32;
  const uint16_t* ap = A + (size_t)(m0 + wm + li) * D + g * 8;
  const uint16_t* bp[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) bp[j] = B + (size_t)(c0 + wn + j * 16 + li) * D + g * 8;
  f32x4 acc[2] = {(f32x4){0.f, 0.f, 0.f, 0.f}, (f32x4){0.f, 0.f, 0.f, 0.f}};
  for (int k = 0; k < D; k += 32) {
    const bf16x8 a = *(const bf16x8*)(ap + k);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const bf16x8 b = *(const bf16x8*)(bp[j] + k);
      acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc[j], 0, 0, 0);
    }
  }
  const float fn = (float)n;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int col = c0 + wn + j * 16 + li;
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = m0 + wm + 4 * g + r;
      const float val = acc[j][r] / fn;
      dzh[(size_t)(v * n + row) * D + col] = val;
      s1 += val;
      s2 += val * bf2f(own[(size_t)row * D + col]);
    }
    s1 += __shfl_xor(s1, 16, 64);
    s1 += __shfl_xor(s1, 32, 64);
    s2 += __shfl_xor(s2, 16, 64);
    s2 += __shfl_xor(s2, 32, 64);
    if (g == 0) {
      red[wid >> 1][0][wn + j * 16 + li] = s1;
      red[wid >> 1][1][wn + j * 16 + li] = s2;
    }
  }
  __syncthreads();
  if (threadIdx.x < 128) {
    const int which = threadIdx.x >> 6, col = threadIdx.x & 63;
    const int MT = n / 32;
    colpart[((size_t)(v * MT + blockIdx.x) * 2 + which) * D + c0 + col] =
        red[0][which][col] + red[1][which][col];
  }
}

// grid (D/64, n/32, 2 views): every block adds its 64 columns' sums of dẑ and of dẑ·ẑ over the
// parts of `sums` in ascending order (the same order in every block) and divides by `rows`, then
// dz = rstd · ((dẑ − m1) − ẑ · m2) for its 32 rows.  sums[v · vstride + p · pstride + which · D + d]:
//   per rank   colpart [2][n/32][2][D]: parts n/32 (row tiles), pstride 2D, vstride (n/32)·2D, rows n
//   all ranks  gsum [W][2][2][D]:       parts W (ranks),        pstride 4D, vstride 2D, rows W·n
__global__ __launch_bounds__(256) void k_bt_std_bwd(const uint16_t* __restrict__ zh,
                                                    const float* __restrict__ rstd,
                                                    const float* __restrict__ dzh,
                                                    const float* __restrict__ sums, int parts,
                                                    int pstride, int vstride, int rows, int n,
                                                    int D, uint16_t* __restrict__ dz_bf16,
                                                    float* __restrict__ dz_f32) {
  __shared__ float m[2][64];
  const int v = blockIdx.z, d0 = blockIdx.x * 64, r0 = blockIdx.y * 32;
  if (threadIdx.x < 128) {
    const int which = threadIdx.x >> 6, col = threadIdx.x & 63;
    const float* src = sums + (size_t)v * vstride + which * D + d0 + col;
    m[which][col] = bt_part_sum(src, parts, pstride) / (float)rows;
  }
  __syncthreads();
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const float m1 = m[0][tx], m2 = m[1][tx];
  const float rs = rstd[(size_t)v * D + d0 + tx];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const size_t i = (size_t)(v * n + r0 + ty * 8 + k) * D + d0 + tx;
    const float val = rs * ((dzh[i] - m1) - bf2f(zh[i]) * m2);
    if (dz_bf16) dz_bf16[i] = f2bf(val);
    if (dz_f32) dz_f32[i] = val;
  }
}

// ---------------------------------------------------------------- the loss over all ranks
// (loss.barlow_global: W ranks of n rows each, N = W·n; contract: loss/barlow.py.)  Between these
// launches the ranks exchange [2][2][D] statistics (all-gather), the D x D slab (all-reduce) and
// [2][2][D] column sums (all-gather); k_bt_corr, k_bt_loss (splits 1, n = N), k_bt_grad, k_bt_bwd
// and k_bt_std_bwd (parts = ranks, rows = N) serve unchanged.

// grid (D/64, 2 views), 1024 threads: the row passes alone; stats[0][v][d] = μ_r,
// stats[1][v][d] = M2_r = Σ_b (z − μ_r)² (not divided)
template <typename T>
__global__ __launch_bounds__(1024) void k_bt_stats(const T* __restrict__ z, int n, int D,
                                                   float* __restrict__ stats) {
  const int v = blockIdx.y, d0 = blockIdx.x * 64;
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  float m2 = 0.f;  // (set by the ty == 0 threads, read by them alone)
  const float mu = bt_row_stats(z + (size_t)v * n * D + d0 + tx, n, D, m2);
  if (ty == 0) {
    stats[(size_t)v * D + d0 + tx] = mu;
    stats[(size_t)(2 + v) * D + d0 + tx] = m2;
  }
}

// grid (D/64, 2 views), 1024 threads.  gst [W][2][2][D] are every rank's statistics in rank order:
// μ = (Σ_r μ_r) / W, M2 = Σ_r (M2_r + n (μ_r − μ)²), both summed in rank order; σ² = M2 / N,
// rstd as k_bt_standardize's, then the write pass on this rank's rows.
// W = 1: μ = μ_0 / 1 and M2 = M2_0 + n · 0, the bits of k_bt_standardize.
template <typename T>
__global__ __launch_bounds__(1024) void k_bt_merge_standardize(const T* __restrict__ z,
                                                               const float* __restrict__ gst,
                                                               int W, int n, int D, float eps,
                                                               float* __restrict__ rstd,
                                                               uint16_t* __restrict__ zh,
                                                               uint16_t* __restrict__ zhT) {
#pragma clang fp contract(off)  // (n · d² and the sum round separately, as the twin's do)
  __shared__ float s_mu[64], s_rs[64];
  const int v = blockIdx.y, d0 = blockIdx.x * 64;
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const T* zv = z + (size_t)v * n * D + d0 + tx;  // (formed here: after the branch it costs VGPRs)
  if (ty == 0) {
    const size_t rank_stride = (size_t)4 * D;
    const float* pm = gst + (size_t)v * D + d0 + tx;        // μ_r
    const float* pq = gst + (size_t)(2 + v) * D + d0 + tx;  // M2_r
    float sm = pm[0];
    for (int r = 1; r < W; ++r) sm += pm[r * rank_stride];
    const float m = div_rn(sm, (float)W);
    const float fn = (float)n;
    float m2 = 0.f;
    for (int r = 0; r < W; ++r) {
      const float d = pm[r * rank_stride] - m;
      const float t = pq[r * rank_stride] + fn * (d * d);
      m2 = r == 0 ? t : m2 + t;
    }
    const float rs = bt_rstd(m2, (float)((long)W * n), eps);
    s_mu[tx] = m;
    s_rs[tx] = rs;
    rstd[(size_t)v * D + d0 + tx] = rs;
  }
  __syncthreads();
  bt_write_zhat(zv, v, d0, n, D, s_mu[tx], s_rs[tx], zh, zhT);
}

// four consecutive entries per thread, as k_bt_loss: S = Σ_s slab_s in split order (not divided)
__global__ __launch_bounds__(256) void k_bt_slab_merge(const float* __restrict__ part, int splits,
                                                       int D, float* __restrict__ S) {
  const size_t i4 = (size_t)blockIdx.x * 256 + threadIdx.x;
  ((float4*)S)[i4] = bt_slab_sum(part, splits, D, i4);
}

// one thread per (view, dẑ | dẑ·ẑ, column), 4 D of them (a multiple of 256): the row tiles'
// partials of k_bt_bwd in tile order, as k_bt_std_bwd sums them per rank; csum [2][2][D]
__global__ __launch_bounds__(256) void k_bt_colsum(const float* __restrict__ colpart, int MT, int D,
                                                   float* __restrict__ csum) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int col = i % D, which = (i / D) & 1, v = i / (2 * D);
  csum[i] = bt_part_sum(colpart + ((size_t)v * MT * 2 + which) * D + col, MT, (size_t)2 * D);
}

}  // namespace

// ------------------------------------------------------------------- host API (raw pointers)
void barlow_standardize(const void* z, int z_f32, int n, int D, float eps, float* rstd,
                        uint16_t* zh, uint16_t* zhT, hipStream_t s) {
  const dim3 grid(D / 64, 2), block(1024);
  if (z_f32)
    hipLaunchKernelGGL(k_bt_standardize<float>, grid, block, 0, s, (const float*)z, n, D, eps,
                       rstd, zh, zhT);
  else
    hipLaunchKernelGGL(k_bt_standardize<uint16_t>, grid, block, 0, s, (const uint16_t*)z, n, D,
                       eps, rstd, zh, zhT);
  HIP_CHECK_LAUNCH();
}

// K = n is split over blocks until about 512 blocks run, at most 16 ways: D 128 has 4 tiles of
// 64 x 64 and takes 16 slices at n 512; from D 1472 on the tiles alone pass 512 and the split is
// 1.  splits <= 512 / tiles + 1 while tiles < 512, so the slabs hold fewer than
// (512 + tiles) · 16 KiB < 16 MiB; at D 2048 they are the one 16 MiB slab.
int barlow_corr_splits(int n, int D) {
  const int tiles = (D / 64) * (D / 64), ksteps = n / 32;
  int want = (512 + tiles - 1) / tiles;
  if (want > 16) want = 16;
  if (want > ksteps) want = ksteps;
  const int per = (ksteps + want - 1) / want;
  return (ksteps + per - 1) / per;  // (no empty slice)
}

void barlow_corr(const uint16_t* zhT, int n, int D, int splits, float* part, hipStream_t s) {
  const int ksteps = n / 32;
  const int kslice = ((ksteps + splits - 1) / splits) * 32;
  hipLaunchKernelGGL(k_bt_corr, dim3(D / 64, D / 64, splits), dim3(256), 0, s, zhT, n, D, kslice,
                     part);
  HIP_CHECK_LAUNCH();
}

int barlow_loss_blocks(int D) { return D * D / 1024; }

void barlow_loss(const float* part, int splits, int n, int D, float lambd, float* C, float* lpart,
                 hipStream_t s) {
  hipLaunchKernelGGL(k_bt_loss, dim3(barlow_loss_blocks(D)), dim3(256), 0, s, part, splits, n, D,
                     lambd, C, lpart);
  HIP_CHECK_LAUNCH();
}

void barlow_grad(const float* C, int D, float lambd, const float* gout, uint16_t* G, uint16_t* GT,
                 hipStream_t s) {
  hipLaunchKernelGGL(k_bt_grad, dim3(D / 64, D / 64), dim3(256), 0, s, C, D, lambd, gout, G, GT);
  HIP_CHECK_LAUNCH();
}

void barlow_backward(const uint16_t* zh, const uint16_t* G, const uint16_t* GT, int n, int D,
                     float* dzh, float* colpart, hipStream_t s) {
  hipLaunchKernelGGL(k_bt_bwd, dim3(n / 32, D / 64, 2), dim3(256), 0, s, zh, G, GT, n, D, dzh,
                     colpart);
  HIP_CHECK_LAUNCH();
}

// the one std-backward launch; the two layouts of `sums` are at k_bt_std_bwd
static void std_backward(const uint16_t* zh, const float* rstd, const float* dzh, const float* sums,
                         int parts, int pstride, int vstride, int rows, int n, int D,
                         uint16_t* dz_bf16, float* dz_f32, hipStream_t s) {
  hipLaunchKernelGGL(k_bt_std_bwd, dim3(D / 64, n / 32, 2), dim3(256), 0, s, zh, rstd, dzh, sums,
                     parts, pstride, vstride, rows, n, D, dz_bf16, dz_f32);
  HIP_CHECK_LAUNCH();
}

void barlow_std_backward(const uint16_t* zh, const float* rstd, const float* dzh,
                         const float* colpart, int n, int D, uint16_t* dz_bf16, float* dz_f32,
                         hipStream_t s) {
  std_backward(zh, rstd, dzh, colpart, n / 32, 2 * D, (n / 32) * 2 * D, n, n, D, dz_bf16, dz_f32, s);
}

// ---- the loss over all ranks (W ranks, N = W · n rows)
void barlow_stats(const void* z, int z_f32, int n, int D, float* stats, hipStream_t s) {
  const dim3 grid(D / 64, 2), block(1024);
  if (z_f32)
    hipLaunchKernelGGL(k_bt_stats<float>, grid, block, 0, s, (const float*)z, n, D, stats);
  else
    hipLaunchKernelGGL(k_bt_stats<uint16_t>, grid, block, 0, s, (const uint16_t*)z, n, D, stats);
  HIP_CHECK_LAUNCH();
}

void barlow_merge_standardize(const void* z, int z_f32, const float* gstats, int W, int n, int D,
                              float eps, float* rstd, uint16_t* zh, uint16_t* zhT,
                              hipStream_t s) {
  const dim3 grid(D / 64, 2), block(1024);
  if (z_f32)
    hipLaunchKernelGGL(k_bt_merge_standardize<float>, grid, block, 0, s, (const float*)z, gstats,
                       W, n, D, eps, rstd, zh, zhT);
  else
    hipLaunchKernelGGL(k_bt_merge_standardize<uint16_t>, grid, block, 0, s, (const uint16_t*)z,
                       gstats, W, n, D, eps, rstd, zh, zhT);
  HIP_CHECK_LAUNCH();
}

void barlow_slab_merge(const float* part, int splits, int D, float* S, hipStream_t s) {
  hipLaunchKernelGGL(k_bt_slab_merge, dim3(barlow_loss_blocks(D)), dim3(256), 0, s, part, splits,
                     D, S);
  HIP_CHECK_LAUNCH();
}

void barlow_colsum(const float* colpart, int n, int D, float* csum, hipStream_t s) {
  hipLaunchKernelGGL(k_bt_colsum, dim3(4 * D / 256), dim3(256), 0, s, colpart, n / 32, D, csum);
  HIP_CHECK_LAUNCH();
}

void barlow_std_backward_global(const uint16_t* zh, const float* rstd, const float* dzh,
                                const float* gsum, int W, int n, int D, uint16_t* dz_bf16,
                                float* dz_f32, hipStream_t s) {
  std_backward(zh, rstd, dzh, gsum, W, 4 * D, 2 * D, W * n, n, D, dz_bf16, dz_f32, s);
}
