// NNCLR (Dwibedi et al., 2021): every embedding is replaced by its nearest neighbour in a FIFO
// support set of past embeddings, and that neighbour is contrasted against the other view
// (loss/nnclr.py has the contract).  Seven launches forward, two backward; no 2n x Q and no
// n x n buffer exists at any point.
//
//   k_nc_normalize  ẑ = z / max(|z|, 1e-12): the norm accumulated in fp64 (order-free, as
//                   k_knn_normalize), the quotient a correctly rounded fp32 division; writes ẑ in
//                   fp32 (for the normalisation backward), ẑ rounded once to bf16 (the operand
//                   of everything else) and 1 / max(|z|, 1e-12).  One wave per row.
//   k_nc_top1       block = one wave, 32 query rows x one split of the queue, on
//                   v_mfma_f32_16x16x32_bf16: the two query tiles stay in registers (B operand),
//                   the queue rows stream through as the A operand, 64 rows per iteration.  Lane
//                   (g, li) sees query li against queue rows 4g + r of every tile and keeps one
//                   running (best similarity, index) pair per query tile; it visits its indices
//                   in ascending order and replaces only on `>`, so ties keep the lowest index and
//                   a NaN never wins.  The four lane groups are merged by (similarity descending,
//                   index ascending), a total order.  One candidate per row and split.
//   k_nc_select     one wave per row: the splits' candidates merged by the same order, idx written,
//                   a = Qm[idx] copied to the saved buffer.
//   k_nc_fwd        block = one wave, 16 anchor rows of view v (their neighbours a in registers) x
//                   one split of the other view's n columns; online log-sum-exp per lane, the
//                   positive picked where column == image; partials in k_ntxent_fwd's format, so
//                   ntxent_finish / ntxent_reduce_loss merge them.
//   k_nc_enqueue    ONE block: every thread reads the cursor, a block barrier, then the n rows of
//                   view 0 go to (cursor + b) mod Q and thread 0 writes the new cursor.  One block,
//                   because no other block may read the cursor after it was advanced; the copy is
//                   n·D·2 bytes (128 KiB at n 512, D 128).
//   k_nc_bwd        the column pass (P − I)ᵀ·A: block = one wave, 16 owned columns (rows of ẑ of
//                   view 1−v, B operand of the similarity tile) x one split of the anchors of view
//                   v; S recomputed on the bf16 MFMA, w = g/(2n)·(exp(s − lse) − [i = c]) in fp32
//                   and contracted with a on v_mfma_f32_16x16x4_f32 (w is not rounded).
//   k_nc_norm_bwd   sums the anchor splits in split order, then the NT-Xent normalisation
//                   backward dz = (dẑ − ẑ (ẑ·dẑ)) / max(|z|, 1e-12).  One wave per row.
//
// Fragment layout of v_mfma_f32_16x16x32_bf16 (as knn.hip): lane (g = lane >> 4, li = lane & 15)
// holds A[m = li][k = 8g .. 8g + 7] and B[n = li][k = 8g .. 8g + 7]; acc[r] = C[m = 4g + r][n = li].
#include <algorithm>

#include "common.h"
#include "contrast.h"
#include "kernels.h"

namespace {

template <typename T> __device__ __forceinline__ float nc_ld(const T* p);
template <> __device__ __forceinline__ float nc_ld<float>(const float* p) { return *p; }
template <> __device__ __forceinline__ float nc_ld<uint16_t>(const uint16_t* p) { return bf2f(*p); }

template <typename T>
__global__ __launch_bounds__(256) void k_nc_normalize(const T* __restrict__ z, int R, int D,
                                                      float* __restrict__ zn,
                                                      uint16_t* __restrict__ zb,
                                                      float* __restrict__ inv_norm) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= R) return;
  const T* src = z + (size_t)row * D;
  double ss = 0.0;
  for (int d = lane; d < D; d += 64) {
    const double v = (double)nc_ld(src + d);
    ss += v * v;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) ss += __shfl_xor(ss, o, 64);
  const float den = fmaxf((float)sqrt(ss), 1e-12f);  // F.normalize eps
  for (int d = lane; d < D; d += 64) {
    const float v = nc_ld(src + d) / den;
    zn[(size_t)row * D + d] = v;
    zb[(size_t)row * D + d] = f2bf(v);
  }
  if (lane == 0) inv_norm[row] = 1.f / den;
}

// (similarity descending, index ascending): whether (v2, i2) comes before (v, i)
__device__ __forceinline__ bool nc_before(float v2, int i2, float v, int i) {
  return v2 > v || (v2 == v && i2 < i);
}

// zb [R][D], Qm [Q][D] bf16.  grid (R / 32, splits); split y owns queue rows
// [y · rows_per_split, ...) (a multiple of 64, clamped to Q).  candv / candi [splits][R].
template <int D>
__global__ __launch_bounds__(64) void k_nc_top1(const uint16_t* __restrict__ zb,
                                                const uint16_t* __restrict__ Qm, int R, int Q,
                                                int rows_per_split, float* __restrict__ candv,
                                                int* __restrict__ candi) {
  constexpr int KS = D / 32;
  const int lane = threadIdx.x, g = lane >> 4, li = lane & 15;
  const int r0 = blockIdx.x * 32;
  const int q_beg = blockIdx.y * rows_per_split;
  const int q_end = min(Q, q_beg + rows_per_split);
  bf16x8 bq[2][KS];
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int ks = 0; ks < KS; ++ks)
      bq[t][ks] = *(const bf16x8*)(zb + (size_t)(r0 + 16 * t + li) * D + ks * 32 + g * 8);
  float best[2] = {-INFINITY, -INFINITY};
  int bidx[2] = {0, 0};
  for (int q0 = q_beg; q0 < q_end; q0 += 64) {
    f32x4 acc[4][2];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int t = 0; t < 2; ++t) acc[j][t] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      bf16x8 a[4];
#pragma unroll
      for (int j = 0; j < 4; ++j)
        a[j] = *(const bf16x8*)(Qm + (size_t)(q0 + 16 * j + li) * D + ks * 32 + g * 8);
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int t = 0; t < 2; ++t)
          acc[j][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[j], bq[t][ks], acc[j][t], 0, 0, 0);
    }
    // ascending queue index per lane: tile j, then row r
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          const float v = acc[j][t][r];
          if (v > best[t]) {
            best[t] = v;
            bidx[t] = q0 + 16 * j + 4 * g + r;
          }
        }
  }
#pragma unroll
  for (int t = 0; t < 2; ++t) {
#pragma unroll
    for (int off = 16; off < 64; off <<= 1) {
      const float v2 = __shfl_xor(best[t], off, 64);
      const int i2 = __shfl_xor(bidx[t], off, 64);
      if (nc_before(v2, i2, best[t], bidx[t])) {
        best[t] = v2;
        bidx[t] = i2;
      }
    }
    if (g == 0) {
      candv[(size_t)blockIdx.y * R + r0 + 16 * t + li] = best[t];
      candi[(size_t)blockIdx.y * R + r0 + 16 * t + li] = bidx[t];
    }
  }
}

// one wave per row: merge the splits, write idx, gather a = Qm[idx] (D / 2 words)
__global__ __launch_bounds__(256) void k_nc_select(const float* __restrict__ candv,
                                                   const int* __restrict__ candi,
                                                   const uint16_t* __restrict__ Qm, int R, int Q,
                                                   int D, int splits, int* __restrict__ idx,
                                                   uint16_t* __restrict__ a) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= R) return;
  float v = -INFINITY;
  int i = 0;
  for (int s = lane; s < splits; s += 64) {
    const float v2 = candv[(size_t)s * R + row];
    const int i2 = candi[(size_t)s * R + row];
    if (nc_before(v2, i2, v, i)) {
      v = v2;
      i = i2;
    }
  }
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const float v2 = __shfl_xor(v, off, 64);
    const int i2 = __shfl_xor(i, off, 64);
    if (nc_before(v2, i2, v, i)) {
      v = v2;
      i = i2;
    }
  }
  i = min(max(i, 0), Q - 1);  // (always in range; a bad candidate must not read outside Qm)
  if (lane == 0) idx[row] = i;
  const uint32_t* src = reinterpret_cast<const uint32_t*>(Qm + (size_t)i * D);
  uint32_t* dst = reinterpret_cast<uint32_t*>(a + (size_t)row * D);
  for (int w = lane; w < D / 2; w += 64) dst[w] = src[w];
}

// S^T tile [partner q (16)][owned o (16)] = Σ_k P[q][k] O[o][k]; lane gets (q = 4g + r, o = li).
// prow: the lane's partner row pointer (row q0 + li, at column 8g); breg: the owned fragments.
template <int D>
__device__ __forceinline__ f32x4 nc_sim_tile(const uint16_t* __restrict__ prow,
                                             const bf16x8* breg) {
  f32x4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = {0.f, 0.f, 0.f, 0.f};
  if constexpr (D == 32) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(*(const bf16x8*)prow, breg[0], a0, 0, 0, 0);
  } else {
#pragma unroll
    for (int ks = 0; ks < D / 32; ks += 2) {
      const bf16x8 p0 = *(const bf16x8*)(prow + ks * 32);
      const bf16x8 p1 = *(const bf16x8*)(prow + (ks + 1) * 32);
      a0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(p0, breg[ks], a0, 0, 0, 0);
      a1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(p1, breg[ks + 1], a1, 0, 0, 0);
    }
    return a0 + a1;
  }
}

// grid (R / 16, splits), one wave.  Owned = anchor rows [r0, r0 + 16) of view v (a in
// registers), partners = columns [c_beg, c_end) of view 1 − v (rows of zb).  part[split][r][3] =
// (max, sumexp, positive logit or −inf), the format of k_ntxent_fwd.
template <int D>
__global__ __launch_bounds__(64) void k_nc_fwd(const uint16_t* __restrict__ a,
                                               const uint16_t* __restrict__ zb, int n,
                                               float inv_temp, int cols_per_split,
                                               float* __restrict__ part) {
  const int lane = threadIdx.x, g = lane >> 4, li = lane & 15;
  const int R = 2 * n;
  const int r0 = blockIdx.x * 16;
  const int v = r0 >= n ? 1 : 0;  // (n % 16 == 0: a tile never straddles the views)
  const int c_beg = blockIdx.y * cols_per_split;
  const int c_end = min(n, c_beg + cols_per_split);
  bf16x8 breg[D / 32];
#pragma unroll
  for (int ks = 0; ks < D / 32; ++ks)
    breg[ks] = *(const bf16x8*)(a + (size_t)(r0 + li) * D + ks * 32 + g * 8);
  const int my_i = r0 + li - v * n;  // the lane's image = its positive column
  const uint16_t* cols = zb + (size_t)(1 - v) * n * D;
  float m = -INFINITY, l = 0.f, spos = -INFINITY;
  for (int q0 = c_beg; q0 < c_end; q0 += 16) {
    const f32x4 s = nc_sim_tile<D>(cols + (size_t)(q0 + li) * D + g * 8, breg);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int c = q0 + 4 * g + i;
      const float x = s[i] * inv_temp;
      if (c == my_i) spos = x;
      lse_push(m, l, x);
    }
  }
#pragma unroll
  for (int off = 16; off < 64; off <<= 1) {
    lse_merge_lanes(m, l, off);
    spos = fmaxf(spos, __shfl_xor(spos, off, 64));
  }
  if (g == 0) {
    float* dst = part + ((size_t)blockIdx.y * R + r0 + li) * 3;
    dst[0] = m;
    dst[1] = l;
    dst[2] = spos;
  }
}

// grid (R / 16, splits), one wave.  Owned = rows [o0, o0 + 16) of zb (view u), as columns of
// the anchors of view v = 1 − u; partners = anchors i in [q_beg, q_end) (rows v·n + i of a).
// out[split][o][d] = (1/τ) Σ_i w(i, o) a[v·n + i][d], w = gs·(exp(s − lse_i) − [i = c_o]).
template <int D>
__global__ __launch_bounds__(64) void k_nc_bwd(const uint16_t* __restrict__ a,
                                               const uint16_t* __restrict__ zb,
                                               const float* __restrict__ lse, int n,
                                               float inv_temp, const float* __restrict__ gout,
                                               int anchors_per_split, float* __restrict__ out) {
  const int lane = threadIdx.x, g = lane >> 4, li = lane & 15;
  const int R = 2 * n;
  const int o0 = blockIdx.x * 16;
  const int u = o0 >= n ? 1 : 0;
  const int v = 1 - u;
  const int q_beg = blockIdx.y * anchors_per_split;
  const int q_end = min(n, q_beg + anchors_per_split);
  const float gs = gout[0] / (float)R;
  bf16x8 breg[D / 32];
#pragma unroll
  for (int ks = 0; ks < D / 32; ++ks)
    breg[ks] = *(const bf16x8*)(zb + (size_t)(o0 + li) * D + ks * 32 + g * 8);
  const int my_c = o0 + li - u * n;  // the owned row as a column of the other view
  const uint16_t* anc = a + (size_t)v * n * D;
  const float* lse_v = lse + (size_t)v * n;
  constexpr int nd = D / 16;
  f32x4 acc[nd];
#pragma unroll
  for (int t = 0; t < nd; ++t) acc[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
  for (int q0 = q_beg; q0 < q_end; q0 += 16) {
    const f32x4 s = nc_sim_tile<D>(anc + (size_t)(q0 + li) * D + g * 8, breg);
    float w[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int q = q0 + 4 * g + i;  // anchor image
      const float p = __expf(s[i] * inv_temp - lse_v[q]);
      w[i] = gs * (p - (q == my_c ? 1.f : 0.f));
    }
    // acc[o][d] += Σ_q w(q, o) a[q][d]: A[o = li][k = g] = w[t] (q = 4g + t), B[k = g][d = li]
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const uint16_t* arow = anc + (size_t)(q0 + 4 * g + t) * D + li;
#pragma unroll
      for (int dt = 0; dt < nd; ++dt)
        acc[dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[t], bf2f(arow[dt * 16]), acc[dt], 0, 0, 0);
    }
  }
  // lane holds out[o = 4g + i][d = 16 dt + li]
  float* dst = out + (size_t)blockIdx.y * R * D;
#pragma unroll
  for (int dt = 0; dt < nd; ++dt)
#pragma unroll
    for (int i = 0; i < 4; ++i)
      dst[(size_t)(o0 + 4 * g + i) * D + dt * 16 + li] = acc[dt][i] * inv_temp;
}

// dẑ = Σ_s part[s] (split order), dz = (dẑ − ẑ (ẑ·dẑ)) · inv_norm; one wave per row
__global__ __launch_bounds__(256) void k_nc_norm_bwd(const float* __restrict__ zn,
                                                     const float* __restrict__ inv_norm,
                                                     const float* __restrict__ part, int splits,
                                                     int R, int D, uint16_t* __restrict__ dz_bf16,
                                                     float* __restrict__ dz_f32) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= R) return;
  float dzn[4];  // D <= 256: at most 4 columns per lane
  float dot = 0.f;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int d = lane + 64 * k;
    float s = 0.f;
    if (d < D) {
      for (int sp = 0; sp < splits; ++sp) s += part[((size_t)sp * R + row) * D + d];
      dot += zn[(size_t)row * D + d] * s;
    }
    dzn[k] = s;
  }
  dot = wave_sum(dot);
  const float inv = inv_norm[row];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int d = lane + 64 * k;
    if (d < D) {
      const size_t i = (size_t)row * D + d;
      const float x = (dzn[k] - zn[i] * dot) * inv;
      if (dz_bf16) dz_bf16[i] = f2bf(x);
      if (dz_f32) dz_f32[i] = x;
    }
  }
}

// ONE block.  rows [0, n) of zb -> Qm[(cursor + b) mod Q], cursor <- (cursor + n) mod Q.
__global__ __launch_bounds__(1024) void k_nc_enqueue(const uint16_t* __restrict__ zb, int n, int D,
                                                     int Q, uint16_t* __restrict__ Qm,
                                                     int* __restrict__ cursor) {
  int cur = cursor[0];
  cur = ((cur % Q) + Q) % Q;  // (a cursor from a damaged file must not write outside Qm)
  __syncthreads();            // every thread holds the old cursor
  const int cpr = D / 8;      // 16-byte chunks per row
  const int total = n * cpr;
  for (int c = threadIdx.x; c < total; c += blockDim.x) {
    const int b = c / cpr, k = c - b * cpr;
    int dst = cur + b;
    if (dst >= Q) dst -= Q;  // (n <= Q: one wrap at most)
    *(u32x4*)(Qm + (size_t)dst * D + k * 8) = *(const u32x4*)(zb + (size_t)b * D + k * 8);
  }
  if (threadIdx.x == 0) cursor[0] = (cur + n) % Q;
}

bool nc_dim_ok(int D) { return D == 32 || D == 64 || D == 128 || D == 256; }

}  // namespace

// ------------------------------------------------------------------- host API (raw pointers)
// Queue splits of the lookup: about four one-wave blocks per CU (1024) over the R / 32 query
// tiles, a whole number of 64-row iterations each, at most 256 (k_nc_select merges them).
int nnclr_top1_splits(int R, int Q) {
  const int qt = R / 32, it = Q / 64;
  int s = (1024 + qt - 1) / qt;
  s = std::max(1, std::min(s, std::min(it, 256)));
  const int per = (it + s - 1) / s;
  return (it + per - 1) / per;  // no empty split
}

// Column (forward) / anchor (backward) splits: at least 512 one-wave blocks over the R / 16
// tiles, each walking at least one 16-wide tile; at most 64 (the backward partials are
// [splits][R][D] fp32).
int nnclr_loss_splits(int n) {
  const int tiles = 2 * n / 16, pt = n / 16;
  int s = (512 + tiles - 1) / tiles;
  s = std::max(1, std::min(s, std::min(pt, 64)));
  const int per = (pt + s - 1) / s;
  return (pt + per - 1) / per;
}

void nnclr_normalize(const void* z, int z_f32, int R, int D, float* zn, uint16_t* zb,
                     float* inv_norm, hipStream_t s) {
  const dim3 grid((R + 3) / 4);
  if (z_f32)
    hipLaunchKernelGGL(k_nc_normalize<float>, grid, dim3(256), 0, s, (const float*)z, R, D, zn, zb,
                       inv_norm);
  else
    hipLaunchKernelGGL(k_nc_normalize<uint16_t>, grid, dim3(256), 0, s, (const uint16_t*)z, R, D,
                       zn, zb, inv_norm);
  HIP_CHECK_LAUNCH();
}

void nnclr_lookup(const uint16_t* zb, const uint16_t* Qm, int R, int Q, int D, int splits,
                  float* candv, int* candi, int* idx, uint16_t* a, hipStream_t s) {
  if (!nc_dim_ok(D) || R % 32 || Q % 64 || splits < 1) {
    fprintf(stderr, "nnclr_lookup: bad sizes R=%d Q=%d D=%d splits=%d\n", R, Q, D, splits);
    abort();
  }
  const int it = Q / 64;
  const int per = ((it + splits - 1) / splits) * 64;
  DISPATCH_D(D, "nnclr", hipLaunchKernelGGL(k_nc_top1<DD>, dim3(R / 32, splits), dim3(64), 0, s,
                                            zb, Qm, R, Q, per, candv, candi));
  HIP_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_nc_select, dim3((R + 3) / 4), dim3(256), 0, s, candv, candi, Qm, R, Q, D,
                     splits, idx, a);
  HIP_CHECK_LAUNCH();
}

void nnclr_forward(const uint16_t* a, const uint16_t* zb, int n, int D, float inv_temp, int splits,
                   float* part, hipStream_t s) {
  if (!nc_dim_ok(D) || n % 16 || splits < 1) {
    fprintf(stderr, "nnclr_forward: bad sizes n=%d D=%d splits=%d\n", n, D, splits);
    abort();
  }
  const int pt = n / 16;
  const int per = ((pt + splits - 1) / splits) * 16;
  DISPATCH_D(D, "nnclr", hipLaunchKernelGGL(k_nc_fwd<DD>, dim3(2 * n / 16, splits), dim3(64), 0,
                                            s, a, zb, n, inv_temp, per, part));
  HIP_CHECK_LAUNCH();
}

void nnclr_backward(const uint16_t* a, const uint16_t* zb, const float* zn, const float* inv_norm,
                    const float* lse, int n, int D, float inv_temp, const float* gout, int splits,
                    float* part, uint16_t* dz_bf16, float* dz_f32, hipStream_t s) {
  if (!nc_dim_ok(D) || n % 16 || splits < 1) {
    fprintf(stderr, "nnclr_backward: bad sizes n=%d D=%d splits=%d\n", n, D, splits);
    abort();
  }
  const int R = 2 * n, pt = n / 16;
  const int per = ((pt + splits - 1) / splits) * 16;
  DISPATCH_D(D, "nnclr", hipLaunchKernelGGL(k_nc_bwd<DD>, dim3(R / 16, splits), dim3(64), 0, s,
                                            a, zb, lse, n, inv_temp, gout, per, part));
  HIP_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_nc_norm_bwd, dim3((R + 3) / 4), dim3(256), 0, s, zn, inv_norm, part, splits,
                     R, D, dz_bf16, dz_f32);
  HIP_CHECK_LAUNCH();
}

void nnclr_enqueue(const uint16_t* zb, int n, int D, int Q, uint16_t* Qm, int* cursor,
                   hipStream_t s) {
  if (n < 1 || n > Q || D % 8) {
    fprintf(stderr, "nnclr_enqueue: bad sizes n=%d Q=%d D=%d\n", n, Q, D);
    abort();
  }
  hipLaunchKernelGGL(k_nc_enqueue, dim3(1), dim3(1024), 0, s, zb, n, D, Q, Qm, cursor);
  HIP_CHECK_LAUNCH();
}
