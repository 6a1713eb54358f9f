// Linear-probe sweep: G linear classifiers (one per (lr, weight decay) of a grid) trained on the
// same shuffled feature batches.  A training step is two launches whatever G is:
//
//   k_probe_fwd           logits = X[idx] · Wshᵀ + b on v_mfma_f32_16x16x32_bf16 with the A operand
//                         gathered through the batch's index vector, then per configuration the
//                         fp32 softmax / cross-entropy over its C columns, the target's rank, and
//                         (training) dlogits = (softmax - onehot) / rows as bf16, transposed
//                         ([column][row], the K-contiguous A operand of the weight gradient), plus
//                         the bias-gradient partial of every 16-row tile in row order.
//                         One wave owns 16 batch rows of one configuration and walks that
//                         configuration's column tiles; the block is four such waves, grid
//                         (row tiles / 4, G).  Logits go through a scratch that only the writing
//                         lane reads back, so there is no barrier and no LDS.
//   k_probe_wgrad_update  dW = bf16(dlogits)ᵀ · X[idx], one block per 64 columns x 64 features
//                         with K = the whole batch (no split-K: one fixed summation order), the
//                         gathered X tile transposed through LDS.  The epilogue applies weight
//                         decay, momentum and the Nesterov update to master and momentum and
//                         refreshes the bf16 shadow; the blocks of the first feature tile also
//                         reduce the bias partials (tile order) and update the bias.
//
// Columns: configuration g owns [g · Cp, g · Cp + C) of G · Cp, Cp = C rounded up to 16.  The
// padding columns take no part in the softmax, get zero dlogits and are skipped by the update.
// Every value of a configuration is computed from that configuration's columns alone in an order
// that depends on (rows, F, C) only, so a trajectory does not depend on G or on the neighbours.
#include <algorithm>

#include "common.h"
#include "kernels.h"

namespace {

constexpr int PR_KSTEP = 64;  // feature padding: the update's feature tile
constexpr int PR_MAX_G = 16, PR_MAX_COLS = 1024, PR_MAX_ROWS = 4096;
constexpr int PR_UN = 64, PR_UF = 64, PR_UK = 32, PR_UKP = PR_UK + 8;

__device__ __forceinline__ long long pr_src(const int64_t* idx, int row, long long N) {
  const long long s = idx[row];
  return s < 0 ? 0 : (s >= N ? N - 1 : s);  // never out of the feature matrix
}

template <int NJ, bool TRAIN>
__global__ __launch_bounds__(256) void k_probe_fwd(ProbeFwdArgs p) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int li = lane & 15, lg = lane >> 4;
  const int rt = blockIdx.x * 4 + wid;  // 16-row tile of this wave
  const int r0 = rt * 16;
  if (r0 >= p.Rp) return;
  const int NT = p.G * p.Cp;
  const int c0 = blockIdx.y * p.Cp;
  const int ntile = p.Cp / 16;

  if (r0 >= p.rows) {  // rows of the K padding only: zero dlogits
    if (TRAIN) {
      for (int j = 0; j < ntile; ++j)
        *(u32x2*)(p.dlT + (size_t)(c0 + 16 * j + li) * p.ldr + r0 + 4 * lg) = (u32x2){0u, 0u};
    }
    return;
  }

  const uint16_t* ap = p.X + (size_t)pr_src(p.idx, min(r0 + li, p.rows - 1), p.N) * p.Fp + lg * 8;
  int tgt[4];
  bool valid[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = r0 + 4 * lg + r;
    valid[r] = row < p.rows;
    const int64_t t = p.y[pr_src(p.idx, min(row, p.rows - 1), p.N)];
    tgt[r] = (t >= 0 && t < p.C) ? (int)t : -1;
  }

  // pass 1: logits to the scratch, row maximum and the target's logit
  float mx[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
  uint32_t ztb[4] = {0u, 0u, 0u, 0u};
  for (int j0 = 0; j0 < ntile; j0 += NJ) {
    f32x4 acc[NJ];
    const uint16_t* bp[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      acc[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
      bp[j] = p.Wsh + (size_t)(c0 + 16 * min(j0 + j, ntile - 1) + li) * p.Fp + lg * 8;
    }
#pragma unroll 4
    for (int kk = 0; kk < p.Fp; kk += 32) {
      const bf16x8 a = *(const bf16x8*)(ap + kk);
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const bf16x8 b = *(const bf16x8*)(bp[j] + kk);
        acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc[j], 0, 0, 0);
      }
    }
    // acc[j][r]: batch row r0 + 4 lg + r, column 16 (j0 + j) + li of the configuration
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int col = 16 * (j0 + j) + li;
      if (j0 + j >= ntile || col >= p.C) continue;
      const float bias = p.bias[c0 + col];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        if (!valid[r]) continue;
        const float z = acc[j][r] + bias;
        p.Z[(size_t)(r0 + 4 * lg + r) * NT + c0 + col] = z;
        mx[r] = fmaxf(mx[r], z);
        if (col == tgt[r]) ztb[r] = __float_as_uint(z);
      }
    }
  }
  float zt[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) {
      mx[r] = fmaxf(mx[r], __shfl_xor(mx[r], o, 64));
      ztb[r] |= __shfl_xor(ztb[r], o, 64);
    }
    zt[r] = tgt[r] >= 0 ? __uint_as_float(ztb[r]) : __builtin_nanf("");
  }

  // pass 2: softmax denominator and the target's rank.  fmaxf drops a NaN, the sum keeps it.
  float se[4] = {0.f, 0.f, 0.f, 0.f};
  int above[4] = {0, 0, 0, 0};
  for (int col = li; col < p.C; col += 16) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      if (!valid[r]) continue;
      const float z = p.Z[(size_t)(r0 + 4 * lg + r) * NT + c0 + col];
      se[r] += expf(z - mx[r]);
      above[r] += (z > zt[r] || (z == zt[r] && col < tgt[r]) || (z != z && col != tgt[r])) ? 1 : 0;
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) {
      se[r] += __shfl_xor(se[r], o, 64);
      above[r] += __shfl_xor(above[r], o, 64);
    }
    if (li == 0 && valid[r]) {
      const int row = r0 + 4 * lg + r;
      p.loss[(size_t)blockIdx.y * p.loss_stride + row] = logf(se[r]) + mx[r] - zt[r];
      if (p.rank) p.rank[(size_t)blockIdx.y * p.rows + row] = (zt[r] != zt[r]) ? p.C : above[r];
    }
  }

  if (!TRAIN) return;
  // pass 3: dlogits (bf16, transposed) and the tile's bias-gradient partial in row order
  const float frows = (float)p.rows;
  for (int j = 0; j < ntile; ++j) {
    const int col = 16 * j + li;
    float d[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      d[r] = 0.f;
      if (valid[r] && col < p.C) {
        const float z = p.Z[(size_t)(r0 + 4 * lg + r) * NT + c0 + col];
        d[r] = (expf(z - mx[r]) / se[r] - (col == tgt[r] ? 1.f : 0.f)) / frows;
      }
    }
    *(u32x2*)(p.dlT + (size_t)(c0 + col) * p.ldr + r0 + 4 * lg) =
        (u32x2){pack2bf(d[0], d[1]), pack2bf(d[2], d[3])};
    float sum = 0.f;
#pragma unroll
    for (int gg = 0; gg < 4; ++gg)
#pragma unroll
      for (int r = 0; r < 4; ++r) sum += __shfl(d[r], gg * 16 + li, 64);
    if (lg == 0) p.dbp[(size_t)rt * NT + c0 + col] = sum;
  }
}

// Nesterov SGD of torch.optim.SGD on one element: returns the new parameter
__device__ __forceinline__ float pr_sgd(float pw, float grad, float* mom_buf, float wd, float lr,
                                        float m, int step) {
  const float g = grad + wd * pw;
  const float buf = step == 0 ? g : m * (*mom_buf) + g;
  *mom_buf = buf;
  return pw - lr * (g + m * buf);
}

__global__ __launch_bounds__(256) void k_probe_wgrad_update(ProbeUpdArgs p) {
  __shared__ __attribute__((aligned(16))) uint16_t Xs[PR_UF * PR_UKP];  // [feature][batch row]
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int li = lane & 15, lg = lane >> 4;
  const int f0 = blockIdx.x * PR_UF, n0 = blockIdx.y * PR_UN;
  const int NT = p.G * p.Cp;
  const int ncnt = min(PR_UN / 16, (NT - n0) / 16);

  // staging: 32 batch rows x 8 16-byte chunks of the feature tile, one chunk per thread
  const int sk = tid >> 3, sc = tid & 7;
  auto load = [&](int k0) -> u32x4 {
    const int k = k0 + sk;
    if (k >= p.rows) return (u32x4){0u, 0u, 0u, 0u};
    return *(const u32x4*)(p.X + (size_t)pr_src(p.idx, k, p.N) * p.Fp + f0 + sc * 8);
  };

  f32x4 acc[PR_UN / 16];
#pragma unroll
  for (int i = 0; i < PR_UN / 16; ++i) acc[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
  u32x4 rx = load(0);
  for (int k0 = 0; k0 < p.Rp; k0 += PR_UK) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      Xs[(sc * 8 + 2 * i) * PR_UKP + sk] = (uint16_t)(rx[i] & 0xffffu);
      Xs[(sc * 8 + 2 * i + 1) * PR_UKP + sk] = (uint16_t)(rx[i] >> 16);
    }
    __syncthreads();
    if (k0 + PR_UK < p.Rp) rx = load(k0 + PR_UK);
    const bf16x8 b = *(const bf16x8*)(Xs + (16 * wid + li) * PR_UKP + lg * 8);
#pragma unroll
    for (int i = 0; i < PR_UN / 16; ++i) {
      if (i < ncnt) {
        const bf16x8 a = *(const bf16x8*)(p.dlT + (size_t)(n0 + 16 * i + li) * p.ldr + k0 + lg * 8);
        acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc[i], 0, 0, 0);
      }
    }
    __syncthreads();
  }

  // acc[i][r]: column n0 + 16 i + 4 lg + r, feature f0 + 16 wid + li
  const float fs = p.ftab[p.step];
  const int f = f0 + 16 * wid + li;
#pragma unroll
  for (int i = 0; i < PR_UN / 16; ++i) {
    if (i >= ncnt) continue;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int n = n0 + 16 * i + 4 * lg + r;
      const int cfg = n / p.Cp;
      if (n - cfg * p.Cp >= p.C) continue;  // padding column: never moves
      const size_t o = (size_t)n * p.Fp + f;
      const float w = pr_sgd(p.W[o], acc[i][r], p.Mw + o, p.wd[cfg], p.lr0[cfg] * fs, p.momentum,
                             p.step);
      p.W[o] = w;
      p.Wsh[o] = f2bf(w);
    }
  }

  if (blockIdx.x == 0 && tid < PR_UN) {
    const int n = n0 + tid;
    const int cfg = n / p.Cp;
    if (n < NT && n - cfg * p.Cp < p.C) {
      const int RT = (p.rows + 15) / 16;
      float g = 0.f;
      for (int t = 0; t < RT; ++t) g += p.dbp[(size_t)t * NT + n];
      p.b[n] = pr_sgd(p.b[n], g, p.Mb + n, p.wd[cfg], p.lr0[cfg] * fs, p.momentum, p.step);
    }
  }
}

}  // namespace

int probe_kstep() { return PR_KSTEP; }
int probe_max_configs() { return PR_MAX_G; }
int probe_max_cols() { return PR_MAX_COLS; }
int probe_max_rows() { return PR_MAX_ROWS; }

void probe_forward(const ProbeFwdArgs& a, hipStream_t s) {
  const dim3 grid((a.Rp / 16 + 3) / 4, a.G), block(256);
  const bool train = a.dlT != nullptr;
  if (a.Cp == 16) {
    if (train) hipLaunchKernelGGL((k_probe_fwd<1, true>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((k_probe_fwd<1, false>), grid, block, 0, s, a);
  } else {
    if (train) hipLaunchKernelGGL((k_probe_fwd<4, true>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((k_probe_fwd<4, false>), grid, block, 0, s, a);
  }
  HIP_CHECK_LAUNCH();
}

void probe_update(const ProbeUpdArgs& a, hipStream_t s) {
  const int NT = a.G * a.Cp;
  const dim3 grid(a.Fp / PR_UF, (NT + PR_UN - 1) / PR_UN);
  hipLaunchKernelGGL(k_probe_wgrad_update, grid, dim3(256), 0, s, a);
  HIP_CHECK_LAUNCH();
}
