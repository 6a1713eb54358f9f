// Geometry probe (uniformity / alignment of Wang & Isola 2020, and the spectrum of the feature
// covariance: effective rank, RankMe, participation ratio) on gfx950.  Both halves are symmetric
// products on v_mfma_f32_16x16x32_bf16 of which only the tiles on or above the diagonal are
// launched; no N x N buffer and no atomics exist at any point.  Contract: ops/geometry.py.
//
//   pair part (operands: the k-NN probe's normalised bf16 rows, [N][Dp])
//     k_geo_pair     block = one 128 x 128 tile (ti <= tj) of the Gram matrix, operands staged
//                    through LDS as in k_knn_topk, the tile consumed in registers: for the pairs
//                    i < j < N it sums e = exp(2t(s - 1)), d = 2 - 2s, d over equal labels, and
//                    counts the pairs and the equal-label pairs.  fp32 sums never leave the tile:
//                    a thread adds its 64 elements in order, the lanes by wave_sum, the four waves
//                    in order (a chain of at most GEO_PAIR_CHAIN roundings).  The tile partials
//                    fpart [tiles][3], ipart [tiles][2] are added in fp64 / int64 in tile order by
//                    the caller after one read-back.  Row labels are held once per tile in LDS;
//                    the label-free instantiation holds no label code.
//   spectrum part (operands: the raw features)
//     k_geo_colsum   fp64 column sums of one chunk of GEO_CHUNK rows: row group ty of 16 adds the
//                    chunk's rows ty, ty + 16, ... in order, then the groups in order.
//     k_geo_center   mu = fp32((sum of the chunk sums in chunk order) / N); c = bf16(x - mu)
//                    rounded once, written transposed through an LDS tile as cT [Dp][Np] (K = the
//                    rows contiguous, Np = N rounded up to 64, padding zero).
//     k_geo_syrk     block = (64 x 64 tile ti <= tj of S = c^T c, split of the chunks): fp32 MFMA
//                    accumulation over one chunk, the chunks of the split added in chunk order in
//                    fp64 registers, slab [splits][tiles][64][64] fp64.
//     k_geo_merge    S = sum of the splits' slabs in split order; the lower triangle is the mirror
//                    of the upper one (of a diagonal tile the entries i <= j are the ones used).
//
// A triangular tile index t maps to (ti, tj) by a binary search over the integer row offsets
// ti * T - ti (ti - 1) / 2 (64-bit): exact for every tile count.
#include <algorithm>

#include "common.h"
#include "kernels.h"

namespace {

constexpr int GEO_BM = 128, GEO_BK = 64, GEO_KP = GEO_BK + 8;  // pair tile (square), K-step
constexpr int GEO_PAIR_CHAIN = 72;   // 63 additions in a thread + 6 across lanes + 3 across waves
constexpr int GEO_CHUNK = 2048;      // rows per fp32 accumulation chunk of the spectrum part
constexpr int GEO_ST = 64;           // S tile (square)
constexpr int GEO_RG = 16;           // row groups of the column-sum block
constexpr int GEO_MAX_DP = 4096;

// (ti, tj), ti <= tj < T, of the t-th tile of the upper triangle in row-major order
__device__ __forceinline__ void geo_tri(long long t, int T, int& ti, int& tj) {
  auto off = [T](long long r) { return r * T - r * (r - 1) / 2; };  // tiles before row r
  int lo = 0, hi = T - 1;  // the largest row with off(row) <= t
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (off(mid) <= t) lo = mid; else hi = mid - 1;
  }
  ti = lo;
  tj = lo + (int)(t - off(lo));
}

// Xn [N][Dp] bf16 (normalised, zero-padded), labels [N] int32 (LAB only).  grid (tiles).
template <bool LAB>
__global__ __launch_bounds__(256) void k_geo_pair(const uint16_t* __restrict__ Xn,
                                                  const int* __restrict__ labels, int N, int Dp,
                                                  int T, float c2t, float* __restrict__ fpart,
                                                  int* __restrict__ ipart) {
  __shared__ __attribute__((aligned(16))) uint16_t lds[2 * GEO_BM * GEO_KP];
  __shared__ int lab_r[LAB ? GEO_BM : 1], lab_c[LAB ? GEO_BM : 1];
  __shared__ float redf[4][3];
  __shared__ int redi[4][2];
  uint16_t* As = lds;
  uint16_t* Bs = lds + GEO_BM * GEO_KP;

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int li = lane & 15, g = lane >> 4;
  const int wm = (wid >> 1) * 64, wn = (wid & 1) * 64;
  int ti, tj;
  geo_tri((long long)blockIdx.x, T, ti, tj);
  const int m0 = ti * GEO_BM, n0 = tj * GEO_BM;

  if (LAB) {
    if (tid < GEO_BM) lab_r[tid] = labels[min(m0 + tid, N - 1)];
    else lab_c[tid - GEO_BM] = labels[min(n0 + tid - GEO_BM, N - 1)];
  }

  // staging: 128 rows x 8 16-byte chunks per operand and K-step, 4 + 4 chunks per thread; rows
  // past N read row N - 1 (masked by index in the epilogue)
  const int sr = tid >> 3, sc = tid & 7;
  const uint16_t* aptr[4];
  const uint16_t* bptr[4];
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    aptr[p] = Xn + (size_t)min(m0 + sr + 32 * p, N - 1) * Dp + sc * 8;
    bptr[p] = Xn + (size_t)min(n0 + sr + 32 * p, N - 1) * Dp + sc * 8;
  }

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
  for (int kk = 0; kk < Dp; kk += GEO_BK) {
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      *(u32x4*)(As + (sr + 32 * p) * GEO_KP + sc * 8) = ra[p];
      *(u32x4*)(Bs + (sr + 32 * p) * GEO_KP + sc * 8) = rb[p];
    }
    __syncthreads();
    if (kk + GEO_BK < Dp) {
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        ra[p] = *(const u32x4*)(aptr[p] + kk + GEO_BK);
        rb[p] = *(const u32x4*)(bptr[p] + kk + GEO_BK);
      }
    }
#pragma unroll
    for (int ks = 0; ks < GEO_BK; ks += 32) {
      bf16x8 a[4], b[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        a[i] = *(const bf16x8*)(As + (wm + i * 16 + li) * GEO_KP + ks + g * 8);
        b[i] = *(const bf16x8*)(Bs + (wn + i * 16 + li) * GEO_KP + ks + g * 8);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[i], b[j], acc[i][j], 0, 0, 0);
    }
    __syncthreads();
  }

  // acc[i][j][r]: row m0 + wm + 16 i + 4 g + r, column n0 + wn + 16 j + li
  float sE = 0.f, sA = 0.f, sS = 0.f;
  int nP = 0, nS = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = wm + i * 16 + 4 * g + r;
      const int gi = m0 + row;
      const int lr = LAB ? lab_r[row] : 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int col = wn + j * 16 + li;
        const int gj = n0 + col;
        if (gi < gj && gj < N) {
          const float s = acc[i][j][r];
          const float d = fmaf(-2.f, s, 2.f);
          sE += expf(c2t * (s - 1.f));
          sA += d;
          nP += 1;
          if (LAB && lr == lab_c[col]) {
            sS += d;
            nS += 1;
          }
        }
      }
    }
  }
  sE = wave_sum(sE);
  sA = wave_sum(sA);
  if (LAB) sS = wave_sum(sS);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    nP += __shfl_xor(nP, o, 64);
    if (LAB) nS += __shfl_xor(nS, o, 64);
  }
  if (lane == 0) {
    redf[wid][0] = sE; redf[wid][1] = sA; redf[wid][2] = sS;
    redi[wid][0] = nP; redi[wid][1] = nS;
  }
  __syncthreads();
  if (tid < 3) fpart[(size_t)blockIdx.x * 3 + tid] =
      ((redf[0][tid] + redf[1][tid]) + redf[2][tid]) + redf[3][tid];
  else if (tid < 5) ipart[(size_t)blockIdx.x * 2 + tid - 3] =
      redi[0][tid - 3] + redi[1][tid - 3] + redi[2][tid - 3] + redi[3][tid - 3];
}

// x [N][D] fp32, csum [chunks][Dp] fp64.  grid (Dp / 64, chunks), 1024 threads: column tx of 64,
// row group ty of 16.  Columns d >= D sum to zero.
__global__ __launch_bounds__(1024) void k_geo_colsum(const float* __restrict__ x, int N, int D,
                                                     int Dp, double* __restrict__ csum) {
  __shared__ double red[GEO_RG][64];
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const int d = blockIdx.x * 64 + tx;
  const int r0 = blockIdx.y * GEO_CHUNK, r1 = min(N, r0 + GEO_CHUNK);
  double s = 0.0;
  if (d < D)
    for (int b = r0 + ty; b < r1; b += GEO_RG) s += (double)x[(size_t)b * D + d];
  red[ty][tx] = s;
  __syncthreads();
  if (ty == 0) {
    double t = 0.0;
    for (int k = 0; k < GEO_RG; ++k) t += red[k][tx];
    csum[(size_t)blockIdx.y * Dp + d] = t;
  }
}

// grid (Dp / 64, Np / 64), 256 threads: mu of the block's 64 columns, then its 64 rows centred,
// rounded and written transposed.  cT [Dp][Np]; rows >= N and columns >= D are zero.
__global__ __launch_bounds__(256) void k_geo_center(const float* __restrict__ x,
                                                    const double* __restrict__ csum, int chunks,
                                                    int N, int D, int Dp, int Np,
                                                    float* __restrict__ mu_out,
                                                    uint16_t* __restrict__ cT) {
  __shared__ float s_mu[64];
  __shared__ uint16_t tile[64][66];  // [row][column]
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const int d0 = blockIdx.x * 64, r0 = blockIdx.y * 64;
  if (ty == 0) {
    double t = 0.0;
    for (int c = 0; c < chunks; ++c) t += csum[(size_t)c * Dp + d0 + tx];
    const float m = (float)(t / (double)N);
    s_mu[tx] = m;
    if (blockIdx.y == 0) mu_out[d0 + tx] = m;
  }
  __syncthreads();
  const float mu = s_mu[tx];
  const int d = d0 + tx;
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    const int r = ty * 16 + k;
    const int b = r0 + r;
    tile[r][tx] = (b < N && d < D) ? f2bf(x[(size_t)b * D + d] - mu) : (uint16_t)0;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    const int c = ty * 16 + k;  // column d0 + c of c = row of cT
    cT[(size_t)(d0 + c) * Np + r0 + tx] = tile[tx][c];
  }
}

// cT [Dp][Np] bf16.  grid (tiles of the upper triangle, splits); split y owns the chunks
// [y · cps, (y + 1) · cps).  slab [splits][tiles][64][64] fp64.
__global__ __launch_bounds__(256) void k_geo_syrk(const uint16_t* __restrict__ cT, int Np, int Td,
                                                  int chunks, int cps, double* __restrict__ slab) {
  __shared__ __attribute__((aligned(16))) uint16_t lds[2 * GEO_ST * GEO_KP];
  uint16_t* As = lds;
  uint16_t* Bs = lds + GEO_ST * GEO_KP;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int li = lane & 15, g = lane >> 4;
  const int wm = (wid >> 1) * 32, wn = (wid & 1) * 32;
  int ti, tj;
  geo_tri((long long)blockIdx.x, Td, ti, tj);
  const int m0 = ti * GEO_ST, n0 = tj * GEO_ST;

  // staging: 64 feature rows x 8 16-byte chunks per operand and K-step, 2 + 2 chunks per thread
  const int sr = tid >> 3, sc = tid & 7;
  const uint16_t* aptr[2];
  const uint16_t* bptr[2];
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    aptr[p] = cT + (size_t)(m0 + sr + 32 * p) * Np + sc * 8;
    bptr[p] = cT + (size_t)(n0 + sr + 32 * p) * Np + sc * 8;
  }

  double acc64[2][2][4];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) acc64[i][j][r] = 0.0;

  const int c0 = blockIdx.y * cps, c1 = min(chunks, c0 + cps);
  for (int c = c0; c < c1; ++c) {
    const int kbeg = c * GEO_CHUNK, kend = min(Np, kbeg + GEO_CHUNK);  // multiples of 64
    f32x4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    u32x4 ra[2], rb[2];
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      ra[p] = *(const u32x4*)(aptr[p] + kbeg);
      rb[p] = *(const u32x4*)(bptr[p] + kbeg);
    }
    for (int kk = kbeg; kk < kend; kk += GEO_BK) {
#pragma unroll
      for (int p = 0; p < 2; ++p) {
        *(u32x4*)(As + (sr + 32 * p) * GEO_KP + sc * 8) = ra[p];
        *(u32x4*)(Bs + (sr + 32 * p) * GEO_KP + sc * 8) = rb[p];
      }
      __syncthreads();
      if (kk + GEO_BK < kend) {
#pragma unroll
        for (int p = 0; p < 2; ++p) {
          ra[p] = *(const u32x4*)(aptr[p] + kk + GEO_BK);
          rb[p] = *(const u32x4*)(bptr[p] + kk + GEO_BK);
        }
      }
#pragma unroll
      for (int ks = 0; ks < GEO_BK; ks += 32) {
        bf16x8 a[2], b[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          a[i] = *(const bf16x8*)(As + (wm + i * 16 + li) * GEO_KP + ks + g * 8);
          b[i] = *(const bf16x8*)(Bs + (wn + i * 16 + li) * GEO_KP + ks + g * 8);
        }
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[i], b[j], acc[i][j], 0, 0, 0);
      }
      __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc64[i][j][r] += (double)acc[i][j][r];
  }

  // acc[i][j][r]: S row m0 + wm + 16 i + 4 g + r, column n0 + wn + 16 j + li
  double* out = slab + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * (GEO_ST * GEO_ST);
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        out[(wm + i * 16 + 4 * g + r) * GEO_ST + wn + j * 16 + li] = acc64[i][j][r];
}

// grid (tiles), 256 threads, 16 entries per thread: S [Dp][Dp] fp64, both triangles
__global__ __launch_bounds__(256) void k_geo_merge(const double* __restrict__ slab, int splits,
                                                   int Td, int Dp, double* __restrict__ S) {
  int ti, tj;
  geo_tri((long long)blockIdx.x, Td, ti, tj);
  const size_t tile_sz = GEO_ST * GEO_ST, split_sz = (size_t)gridDim.x * tile_sz;
  const double* src = slab + (size_t)blockIdx.x * tile_sz;
  for (int e = threadIdx.x; e < GEO_ST * GEO_ST; e += 256) {
    const int r = e >> 6, c = e & 63;
    if (ti == tj && r > c) continue;
    double v = src[e];
    for (int s = 1; s < splits; ++s) v += src[(size_t)s * split_sz + e];
    const size_t gi = (size_t)ti * GEO_ST + r, gj = (size_t)tj * GEO_ST + c;
    S[gi * Dp + gj] = v;
    S[gj * Dp + gi] = v;
  }
}

}  // namespace

int geo_kstep() { return GEO_BK; }
int geo_max_dp() { return GEO_MAX_DP; }
int geo_chunk() { return GEO_CHUNK; }
int geo_pair_chain() { return GEO_PAIR_CHAIN; }

long long geo_pair_tiles(int N) {
  const long long T = (N + GEO_BM - 1) / GEO_BM;
  return T * (T + 1) / 2;
}

int geo_syrk_tiles(int Dp) {
  const int Td = Dp / GEO_ST;
  return Td * (Td + 1) / 2;
}

// The chunks are split over blocks until about 512 blocks run (barlow_corr_splits' rule): from
// Dp 2048 on the 528 tiles of the triangle alone pass 512 and nothing is split.  While
// tiles < 512, splits <= 512 / tiles + 1, so the slabs hold fewer than (512 + tiles) · 32 KiB.
int geo_syrk_splits(int N, int Dp) {
  const int tiles = geo_syrk_tiles(Dp), chunks = (N + GEO_CHUNK - 1) / GEO_CHUNK;
  const int want = std::min((512 + tiles - 1) / tiles, chunks);
  const int per = (chunks + want - 1) / want;
  return (chunks + per - 1) / per;  // (no empty split)
}

void geo_pair(const uint16_t* Xn, const int* labels, int N, int Dp, float c2t, float* fpart,
              int* ipart, hipStream_t s) {
  const int T = (N + GEO_BM - 1) / GEO_BM;
  const dim3 grid((unsigned)geo_pair_tiles(N));
  if (labels)
    hipLaunchKernelGGL(k_geo_pair<true>, grid, dim3(256), 0, s, Xn, labels, N, Dp, T, c2t, fpart,
                       ipart);
  else
    hipLaunchKernelGGL(k_geo_pair<false>, grid, dim3(256), 0, s, Xn, labels, N, Dp, T, c2t, fpart,
                       ipart);
  HIP_CHECK_LAUNCH();
}

void geo_center(const float* x, int N, int D, int Dp, int Np, double* csum, float* mu,
                uint16_t* cT, hipStream_t s) {
  const int chunks = (N + GEO_CHUNK - 1) / GEO_CHUNK;
  hipLaunchKernelGGL(k_geo_colsum, dim3(Dp / 64, chunks), dim3(1024), 0, s, x, N, D, Dp, csum);
  HIP_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_geo_center, dim3(Dp / 64, Np / 64), dim3(256), 0, s, x, csum, chunks, N, D,
                     Dp, Np, mu, cT);
  HIP_CHECK_LAUNCH();
}

void geo_syrk(const uint16_t* cT, int N, int Dp, int Np, double* slab, double* S, hipStream_t s) {
  const int Td = Dp / GEO_ST, tiles = geo_syrk_tiles(Dp);
  const int chunks = (N + GEO_CHUNK - 1) / GEO_CHUNK, splits = geo_syrk_splits(N, Dp);
  const int cps = (chunks + splits - 1) / splits;
  hipLaunchKernelGGL(k_geo_syrk, dim3(tiles, splits), dim3(256), 0, s, cT, Np, Td, chunks, cps,
                     slab);
  HIP_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_geo_merge, dim3(tiles), dim3(256), 0, s, slab, splits, Td, Dp, S);
  HIP_CHECK_LAUNCH();
}
