// Online linear probe: one linear classifier trained on the encoder output of every pre-training
// step, inside the captured step.  Everything that changes from step to step (features, labels,
// weights, learning rate, metric accumulators) is read from device memory, so a replayed graph
// trains on the batch of the replay.  A step is four launches of this file plus lr_step:
//
//   k_oprobe_fwd      logits = H · Wshᵀ + b on v_mfma_f32_16x16x32_bf16 (H [rows][Fp] bf16, row r
//                     has label y[r mod n]), the fp32 softmax / cross-entropy over the C columns,
//                     the target's rank, dlogits = (softmax - onehot) / rows as bf16, transposed
//                     ([column][row], the K-contiguous A operand of the weight gradient), and the
//                     bias-gradient partial of every 16-row tile in row order.  One wave owns 16
//                     rows and walks the column tiles; logits go through a scratch that only the
//                     writing lane reads back, so there is no barrier and no LDS.
//   k_oprobe_metrics  one block adds the step's rows to the accumulators in a fixed order: loss
//                     sum (fp64), top-1 count, top-k count, row count (int64).  No atomics.
//   k_oprobe_wgrad    dW = bf16(dlogits)ᵀ · H, one block per 64 columns x 64 features with K = all
//                     rows (no split-K: one fixed summation order), the H tile transposed through
//                     LDS; the blocks of the first feature tile reduce the bias partials in tile
//                     order.  Both go to the flat gradient [Cp · Fp + Cp].
//   k_oprobe_update   torch.optim.SGD(nesterov=True) on the flat master / momentum with the
//                     learning rate of the probe's LR cell, and the bf16 shadow of the weights.
//
// Padding columns (>= C) take no part in the softmax, get zero dlogits and are skipped by the
// update, as are the padding features (>= F).
#include "common.h"
#include "kernels.h"

namespace {

constexpr int OP_KSTEP = 64;  // feature padding: the weight gradient's feature tile
constexpr int OP_MAX_COLS = 1024, OP_MAX_FP = 4096, OP_MAX_ROWS = 8192;
constexpr int OP_UN = 64, OP_UF = 64, OP_UK = 32, OP_UKP = OP_UK + 8;

template <int NJ>
__global__ __launch_bounds__(256) void k_oprobe_fwd(OnlineProbeFwdArgs p) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int li = lane & 15, lg = lane >> 4;
  const int rt = blockIdx.x * 4 + wid;  // 16-row tile of this wave
  const int r0 = rt * 16;
  if (r0 >= p.Rp) return;
  const int ntile = p.Cp / 16;

  if (r0 >= p.rows) {  // the K padding of the weight gradient (rows is a multiple of 16): zeros
    for (int j = 0; j < ntile; ++j)
      *(u32x2*)(p.dlT + (size_t)(16 * j + li) * p.Rp + r0 + 4 * lg) = (u32x2){0u, 0u};
    return;
  }

  const uint16_t* ap = p.X + (size_t)(r0 + li) * p.Fp + lg * 8;
  int tgt[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int t = p.y[(r0 + 4 * lg + r) % p.n];
    tgt[r] = (t >= 0 && t < p.C) ? t : -1;
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
      bp[j] = p.Wsh + (size_t)(16 * min(j0 + j, ntile - 1) + li) * p.Fp + lg * 8;
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
    // acc[j][r]: row r0 + 4 lg + r, column 16 (j0 + j) + li
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int col = 16 * (j0 + j) + li;
      if (j0 + j >= ntile || col >= p.C) continue;
      const float bias = p.bias[col];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float z = acc[j][r] + bias;
        p.Z[(size_t)(r0 + 4 * lg + r) * p.Cp + col] = z;
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
      const float z = p.Z[(size_t)(r0 + 4 * lg + r) * p.Cp + col];
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
    if (li == 0) {
      const int row = r0 + 4 * lg + r;
      p.loss[row] = logf(se[r]) + mx[r] - zt[r];
      p.rank[row] = (zt[r] != zt[r]) ? p.C : above[r];
    }
  }

  // pass 3: dlogits (bf16, transposed) and the tile's bias-gradient partial in row order
  const float frows = (float)p.rows;
  for (int j = 0; j < ntile; ++j) {
    const int col = 16 * j + li;
    float d[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      d[r] = 0.f;
      if (col < p.C) {
        const float z = p.Z[(size_t)(r0 + 4 * lg + r) * p.Cp + col];
        d[r] = (expf(z - mx[r]) / se[r] - (col == tgt[r] ? 1.f : 0.f)) / frows;
      }
    }
    *(u32x2*)(p.dlT + (size_t)col * p.Rp + r0 + 4 * lg) =
        (u32x2){pack2bf(d[0], d[1]), pack2bf(d[2], d[3])};
    float sum = 0.f;
#pragma unroll
    for (int gg = 0; gg < 4; ++gg)
#pragma unroll
      for (int r = 0; r < 4; ++r) sum += __shfl(d[r], gg * 16 + li, 64);
    if (lg == 0) p.dbp[(size_t)rt * p.Cp + col] = sum;
  }
}

// One block: thread t sums the rows t, t + 256, ... in row order, then a binary tree over the
// threads.  The order depends on the row count only.
__global__ __launch_bounds__(256) void k_oprobe_metrics(const float* loss, const int* rank,
                                                         int rows, int top_k, double* acc_loss,
                                                         long long* acc_cnt) {
  __shared__ double sl[256];
  __shared__ int s1[256], sk[256];
  const int tid = threadIdx.x;
  double l = 0.0;
  int c1 = 0, ck = 0;
  for (int r = tid; r < rows; r += 256) {
    l += (double)loss[r];
    const int rk = rank[r];
    c1 += rk == 0 ? 1 : 0;
    ck += rk < top_k ? 1 : 0;
  }
  sl[tid] = l;
  s1[tid] = c1;
  sk[tid] = ck;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) {
      sl[tid] += sl[tid + o];
      s1[tid] += s1[tid + o];
      sk[tid] += sk[tid + o];
    }
    __syncthreads();
  }
  if (tid == 0) {
    acc_loss[0] += sl[0];
    acc_cnt[0] += s1[0];
    acc_cnt[1] += sk[0];
    acc_cnt[2] += rows;
  }
}

__global__ __launch_bounds__(256) void k_oprobe_wgrad(OnlineProbeGradArgs p) {
  __shared__ __attribute__((aligned(16))) uint16_t Xs[OP_UF * OP_UKP];  // [feature][row]
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int li = lane & 15, lg = lane >> 4;
  const int f0 = blockIdx.x * OP_UF, n0 = blockIdx.y * OP_UN;
  const int ncnt = min(OP_UN / 16, (p.Cp - n0) / 16);

  // staging: 32 rows x 8 16-byte chunks of the feature tile, one chunk per thread
  const int sk = tid >> 3, sc = tid & 7;
  auto load = [&](int k0) -> u32x4 {
    const int k = k0 + sk;
    if (k >= p.rows) return (u32x4){0u, 0u, 0u, 0u};
    return *(const u32x4*)(p.X + (size_t)k * p.Fp + f0 + sc * 8);
  };

  f32x4 acc[OP_UN / 16];
#pragma unroll
  for (int i = 0; i < OP_UN / 16; ++i) acc[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
  u32x4 rx = load(0);
  for (int k0 = 0; k0 < p.Rp; k0 += OP_UK) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      Xs[(sc * 8 + 2 * i) * OP_UKP + sk] = (uint16_t)(rx[i] & 0xffffu);
      Xs[(sc * 8 + 2 * i + 1) * OP_UKP + sk] = (uint16_t)(rx[i] >> 16);
    }
    __syncthreads();
    if (k0 + OP_UK < p.Rp) rx = load(k0 + OP_UK);
    const bf16x8 b = *(const bf16x8*)(Xs + (16 * wid + li) * OP_UKP + lg * 8);
#pragma unroll
    for (int i = 0; i < OP_UN / 16; ++i) {
      if (i < ncnt) {
        const bf16x8 a = *(const bf16x8*)(p.dlT + (size_t)(n0 + 16 * i + li) * p.Rp + k0 + lg * 8);
        acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc[i], 0, 0, 0);
      }
    }
    __syncthreads();
  }

  // acc[i][r]: column n0 + 16 i + 4 lg + r, feature f0 + 16 wid + li
  const int f = f0 + 16 * wid + li;
#pragma unroll
  for (int i = 0; i < OP_UN / 16; ++i) {
    if (i >= ncnt) continue;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int n = n0 + 16 * i + 4 * lg + r;
      p.grad[(size_t)n * p.Fp + f] = acc[i][r];
    }
  }

  if (blockIdx.x == 0 && tid < OP_UN) {
    const int n = n0 + tid;
    if (n < p.Cp) {
      const int RT = p.rows / 16;
      float g = 0.f;
      for (int t = 0; t < RT; ++t) g += p.dbp[(size_t)t * p.Cp + n];
      p.grad[(size_t)p.Cp * p.Fp + n] = g;
    }
  }
}

__global__ __launch_bounds__(256) void k_oprobe_update(OnlineProbeUpdArgs p) {
  const int nw = p.Cp * p.Fp;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= nw + p.Cp) return;
  if (i < nw) {
    const int col = i / p.Fp;
    if (col >= p.C || i - col * p.Fp >= p.F) return;  // padding: never moves
  } else if (i - nw >= p.C) {
    return;
  }
  const float lr = p.lr[0];
  const float pv = p.master[i];
  const float d = p.grad[i] * p.gscale + p.wd * pv;
  const float b = p.momentum * p.mom[i] + d;  // mom starts at 0 == torch's buf = clone(d)
  p.mom[i] = b;
  const float np = pv - lr * (d + p.momentum * b);
  p.master[i] = np;
  if (i < nw) p.shadow[i] = f2bf(np);
}

}  // namespace

int online_probe_kstep() { return OP_KSTEP; }
int online_probe_max_cols() { return OP_MAX_COLS; }
int online_probe_max_fp() { return OP_MAX_FP; }
int online_probe_max_rows() { return OP_MAX_ROWS; }

void online_probe_forward(const OnlineProbeFwdArgs& a, hipStream_t s) {
  const dim3 grid((a.Rp / 16 + 3) / 4), block(256);
  if (a.Cp == 16) hipLaunchKernelGGL((k_oprobe_fwd<1>), grid, block, 0, s, a);
  else hipLaunchKernelGGL((k_oprobe_fwd<4>), grid, block, 0, s, a);
  HIP_CHECK_LAUNCH();
}

void online_probe_metrics(const float* loss, const int* rank, int rows, int top_k,
                          double* acc_loss, long long* acc_cnt, hipStream_t s) {
  hipLaunchKernelGGL(k_oprobe_metrics, dim3(1), dim3(256), 0, s, loss, rank, rows, top_k, acc_loss,
                     acc_cnt);
  HIP_CHECK_LAUNCH();
}

void online_probe_wgrad(const OnlineProbeGradArgs& a, hipStream_t s) {
  const dim3 grid(a.Fp / OP_UF, (a.Cp + OP_UN - 1) / OP_UN);
  hipLaunchKernelGGL(k_oprobe_wgrad, grid, dim3(256), 0, s, a);
  HIP_CHECK_LAUNCH();
}

void online_probe_update(const OnlineProbeUpdArgs& a, hipStream_t s) {
  const int total = a.Cp * a.Fp + a.Cp;
  hipLaunchKernelGGL(k_oprobe_update, dim3((total + 255) / 256), dim3(256), 0, s, a);
  HIP_CHECK_LAUNCH();
}
