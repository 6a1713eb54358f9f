// Linear probes: the sweep (G linear classifiers, one per (lr, weight decay) of a grid, trained on
// the same shuffled batches of frozen features) and the online probe (one classifier trained on
// the encoder output of every pre-training step, inside the captured step).  Both run the same two
// kernels; a policy says where a row comes from and where a result goes.
//
//   k_linear_ce_fwd   logits = X[row] · Wshᵀ + b on v_mfma_f32_16x16x32_bf16, then the fp32 softmax /
//                     cross-entropy over the C columns of a configuration, the target's rank, and
//                     (training) dlogits = (softmax - onehot) / rows as bf16, transposed
//                     ([column][row], the K-contiguous A operand of the weight gradient), plus
//                     the bias-gradient partial of every 16-row tile in row order.
//                     One wave owns 16 batch rows of one configuration and walks that
//                     configuration's column tiles; the block is four such waves, grid
//                     (row tiles / 4, configurations).  Logits go through a scratch that only the
//                     writing lane reads back, so there is no barrier and no LDS.
//                       SweepRows   rows gathered through the batch's index vector, int64 labels
//                                   by source row, a ragged last tile, configuration blockIdx.y of
//                                   G; the evaluation variant (no gradients) is compiled apart.
//                       OnlineRows  row r of H with label y[r mod n], rows a multiple of 16, one
//                                   configuration.
//   k_linear_wgrad    dW = bf16(dlogits)ᵀ · X[row], one block per 64 columns x 64 features with
//                     K = the whole batch (no split-K: one fixed summation order), the X tile
//                     transposed through LDS (xt_load / xt_store); the blocks of the first feature
//                     tile also reduce the bias partials in tile order.
//                       GatherRows + SgdEpilogue    the sweep: weight decay, momentum and the
//                                   Nesterov update applied to master and momentum in place, the
//                                   bf16 shadow refreshed.
//                       DirectRows + StoreEpilogue  the online probe: dW and db to the flat
//                                   gradient [Cp · Fp + Cp], which may be all-reduced before
//                                   k_oprobe_update.
//   k_oprobe_metrics  one block adds the step's rows to the accumulators in a fixed order: loss
//                     sum (fp64), top-1 count, top-k count, row count (int64).  No atomics.
//   k_oprobe_update   torch.optim.SGD(nesterov=True) on the flat master / momentum with the
//                     learning rate of the probe's LR cell, and the bf16 shadow of the weights.
//
// Columns: configuration g owns [g · Cp, g · Cp + C) of G · Cp, Cp = C rounded up to 16.  The
// padding columns take no part in the softmax, get zero dlogits and are skipped by the update (as
// are the online probe's padding features).  Every value of a configuration is computed from that
// configuration's columns alone in an order that depends on (rows, F, C) only, so a trajectory
// does not depend on G or on the neighbours, and the two probes agree bit for bit.  Whatever
// changes from step to step of the online probe is read from device memory, so a replayed graph
// trains on the batch of the replay.
#include <algorithm>

#include "common.h"
#include "kernels.h"

namespace {

constexpr int PR_KSTEP = 64;  // feature padding: the weight gradient's feature tile
constexpr int PR_MAX_G = 16, PR_MAX_COLS = 1024, PR_MAX_ROWS = 4096;
constexpr int OP_MAX_COLS = 1024, OP_MAX_FP = 4096, OP_MAX_ROWS = 8192;
constexpr int PR_UN = 64, PR_UF = 64, PR_UK = XT_ROWS, PR_UKP = XT_LD;

__device__ __forceinline__ long long pr_src(const int64_t* idx, int row, long long N) {
  const long long s = idx[row];
  return s < 0 ? 0 : (s >= N ? N - 1 : s);  // never out of the feature matrix
}

// ---- row policies of the forward: built per lane from the kernel's arguments
template <bool TRAIN>
struct SweepRows {
  using Args = ProbeFwdArgs;
  static constexpr bool GRAD = TRAIN;
  const Args& p;
  __device__ __forceinline__ long long src(int row) const {
    return pr_src(p.idx, min(row, p.rows - 1), p.N);
  }
  __device__ __forceinline__ const uint16_t* x(int row) const { return p.X + (size_t)src(row) * p.Fp; }
  __device__ __forceinline__ int target(int row) const {
    const int64_t t = p.y[src(row)];
    return (t >= 0 && t < p.C) ? (int)t : -1;
  }
  __device__ __forceinline__ bool valid(int row) const { return row < p.rows; }
  __device__ __forceinline__ int col0() const { return blockIdx.y * p.Cp; }
  __device__ __forceinline__ int cols() const { return p.G * p.Cp; }
  __device__ __forceinline__ int ldr() const { return p.ldr; }
  __device__ __forceinline__ void store(int row, float loss, int rank) const {
    p.loss[(size_t)blockIdx.y * p.loss_stride + row] = loss;
    if (p.rank) p.rank[(size_t)blockIdx.y * p.rows + row] = rank;
  }
};

struct OnlineRows {
  using Args = OnlineProbeFwdArgs;
  static constexpr bool GRAD = true;
  const Args& p;
  __device__ __forceinline__ const uint16_t* x(int row) const { return p.X + (size_t)row * p.Fp; }
  __device__ __forceinline__ int target(int row) const {
    const int t = p.y[row % p.n];
    return (t >= 0 && t < p.C) ? t : -1;
  }
  __device__ __forceinline__ constexpr bool valid(int) const { return true; }
  __device__ __forceinline__ constexpr int col0() const { return 0; }
  __device__ __forceinline__ int cols() const { return p.Cp; }
  __device__ __forceinline__ int ldr() const { return p.Rp; }
  __device__ __forceinline__ void store(int row, float loss, int rank) const {
    p.loss[row] = loss;
    p.rank[row] = rank;
  }
};

template <int NJ, class Rows>
__global__ __launch_bounds__(256) void k_linear_ce_fwd(typename Rows::Args p) {
  const Rows rw{p};
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int li = lane & 15, lg = lane >> 4;
  const int rt = blockIdx.x * 4 + wid;  // 16-row tile of this wave
  const int r0 = rt * 16;
  if (r0 >= p.Rp) return;
  const int NT = rw.cols(), c0 = rw.col0(), ldr = rw.ldr();
  const int ntile = p.Cp / 16;

  if (r0 >= p.rows) {  // rows of the weight gradient's K padding only: zero dlogits
    if (Rows::GRAD) {
      for (int j = 0; j < ntile; ++j)
        *(u32x2*)(p.dlT + (size_t)(c0 + 16 * j + li) * ldr + r0 + 4 * lg) = (u32x2){0u, 0u};
    }
    return;
  }

  const uint16_t* ap = rw.x(r0 + li) + lg * 8;
  int tgt[4];
  bool valid[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = r0 + 4 * lg + r;
    valid[r] = rw.valid(row);
    tgt[r] = rw.target(row);
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
    if (li == 0 && valid[r])
      rw.store(r0 + 4 * lg + r, logf(se[r]) + mx[r] - zt[r], (zt[r] != zt[r]) ? p.C : above[r]);
  }

  if (!Rows::GRAD) return;
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
    *(u32x2*)(p.dlT + (size_t)(c0 + col) * ldr + r0 + 4 * lg) =
        (u32x2){pack2bf(d[0], d[1]), pack2bf(d[2], d[3])};
    float sum = 0.f;
#pragma unroll
    for (int gg = 0; gg < 4; ++gg)
#pragma unroll
      for (int r = 0; r < 4; ++r) sum += __shfl(d[r], gg * 16 + li, 64);
    if (lg == 0) p.dbp[(size_t)rt * NT + c0 + col] = sum;
  }
}

// ---- row policies and epilogues of the weight gradient
struct GatherRows {
  using Args = ProbeUpdArgs;
  const Args& p;
  __device__ __forceinline__ const uint16_t* x(int k) const {
    return p.X + (size_t)pr_src(p.idx, k, p.N) * p.Fp;
  }
  __device__ __forceinline__ int cols() const { return p.G * p.Cp; }
  __device__ __forceinline__ int ldr() const { return p.ldr; }
  __device__ __forceinline__ int tiles() const { return (p.rows + 15) / 16; }  // bias partials
};

struct DirectRows {
  using Args = OnlineProbeGradArgs;
  const Args& p;
  __device__ __forceinline__ const uint16_t* x(int k) const { return p.X + (size_t)k * p.Fp; }
  __device__ __forceinline__ int cols() const { return p.Cp; }
  __device__ __forceinline__ int ldr() const { return p.Rp; }
  __device__ __forceinline__ int tiles() const { return p.rows / 16; }
};

// Nesterov SGD of torch.optim.SGD on one element: returns the new parameter.  Every multiply-add
// is one fused operation, spelled out so that the bits do not hang on what the optimizer contracts.
__device__ __forceinline__ float pr_sgd(float pw, float grad, float* mom_buf, float wd, float lr,
                                        float m, int step) {
  const float g = fmaf(wd, pw, grad);
  const float buf = step == 0 ? g : fmaf(m, *mom_buf, g);
  *mom_buf = buf;
  return fmaf(-lr, fmaf(m, buf, g), pw);
}

// column n's gradient: weight(n, f, dW[n][f]) per element, bias(n, db[n]) once; moves(n) first
struct SgdEpilogue {
  const ProbeUpdArgs& p;
  const float fs;  // the schedule's factor of this step
  __device__ __forceinline__ SgdEpilogue(const ProbeUpdArgs& p) : p(p), fs(p.ftab[p.step]) {}
  __device__ __forceinline__ bool moves(int n) const {  // a padding column never does
    const int cfg = n / p.Cp;
    return n - cfg * p.Cp < p.C;
  }
  __device__ __forceinline__ void weight(int n, int f, float g) const {
    const int cfg = n / p.Cp;
    const size_t o = (size_t)n * p.Fp + f;
    const float w = pr_sgd(p.W[o], g, p.Mw + o, p.wd[cfg], p.lr0[cfg] * fs, p.momentum, p.step);
    p.W[o] = w;
    p.Wsh[o] = f2bf(w);
  }
  __device__ __forceinline__ void bias(int n, float g) const {
    const int cfg = n / p.Cp;
    p.b[n] = pr_sgd(p.b[n], g, p.Mb + n, p.wd[cfg], p.lr0[cfg] * fs, p.momentum, p.step);
  }
};

struct StoreEpilogue {
  const OnlineProbeGradArgs& p;
  __device__ __forceinline__ StoreEpilogue(const OnlineProbeGradArgs& p) : p(p) {}
  __device__ __forceinline__ constexpr bool moves(int) const { return true; }
  __device__ __forceinline__ void weight(int n, int f, float g) const {
    p.grad[(size_t)n * p.Fp + f] = g;
  }
  __device__ __forceinline__ void bias(int n, float g) const { p.grad[(size_t)p.Cp * p.Fp + n] = g; }
};

template <class Rows, class Epilogue>
__global__ __launch_bounds__(256) void k_linear_wgrad(typename Rows::Args p) {
  __shared__ __attribute__((aligned(16))) uint16_t Xs[PR_UF * PR_UKP];  // [feature][batch row]
  const Rows rw{p};
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int li = lane & 15, lg = lane >> 4;
  const int f0 = blockIdx.x * PR_UF, n0 = blockIdx.y * PR_UN;
  const int NT = rw.cols(), ldr = rw.ldr();
  const int ncnt = min(PR_UN / 16, (NT - n0) / 16);

  // staging: 32 batch rows x 8 16-byte chunks of the feature tile, one chunk per thread
  auto load = [&](int k0) -> u32x4 {
    return xt_load(k0, p.rows, tid, [&](int k) { return rw.x(k) + f0; });
  };

  f32x4 acc[PR_UN / 16];
#pragma unroll
  for (int i = 0; i < PR_UN / 16; ++i) acc[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
  u32x4 rx = load(0);
  for (int k0 = 0; k0 < p.Rp; k0 += PR_UK) {
    xt_store(Xs, tid, rx);
    __syncthreads();
    if (k0 + PR_UK < p.Rp) rx = load(k0 + PR_UK);
    const bf16x8 b = *(const bf16x8*)(Xs + (16 * wid + li) * PR_UKP + lg * 8);
#pragma unroll
    for (int i = 0; i < PR_UN / 16; ++i) {
      if (i < ncnt) {
        const bf16x8 a = *(const bf16x8*)(p.dlT + (size_t)(n0 + 16 * i + li) * ldr + k0 + lg * 8);
        acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc[i], 0, 0, 0);
      }
    }
    __syncthreads();
  }

  // acc[i][r]: column n0 + 16 i + 4 lg + r, feature f0 + 16 wid + li
  const Epilogue ep(p);
  const int f = f0 + 16 * wid + li;
#pragma unroll
  for (int i = 0; i < PR_UN / 16; ++i) {
    if (i >= ncnt) continue;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int n = n0 + 16 * i + 4 * lg + r;
      if (ep.moves(n)) ep.weight(n, f, acc[i][r]);
    }
  }

  if (blockIdx.x == 0 && tid < PR_UN) {
    const int n = n0 + tid;
    if (n < NT && ep.moves(n)) {
      const int RT = rw.tiles();
      float g = 0.f;
      for (int t = 0; t < RT; ++t) g += p.dbp[(size_t)t * NT + n];
      ep.bias(n, g);
    }
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

int probe_kstep() { return PR_KSTEP; }
int probe_max_configs() { return PR_MAX_G; }
int probe_max_cols() { return PR_MAX_COLS; }
int probe_max_rows() { return PR_MAX_ROWS; }
int online_probe_kstep() { return PR_KSTEP; }
int online_probe_max_cols() { return OP_MAX_COLS; }
int online_probe_max_fp() { return OP_MAX_FP; }
int online_probe_max_rows() { return OP_MAX_ROWS; }

// NJ column tiles per pass over the features: 1 iff the configuration is one tile wide
template <class Rows>
static void launch_ce_fwd(const typename Rows::Args& a, int G, hipStream_t s) {
  const dim3 grid((a.Rp / 16 + 3) / 4, G), block(256);
  if (a.Cp == 16) hipLaunchKernelGGL((k_linear_ce_fwd<1, Rows>), grid, block, 0, s, a);
  else hipLaunchKernelGGL((k_linear_ce_fwd<4, Rows>), grid, block, 0, s, a);
  HIP_CHECK_LAUNCH();
}

template <class Rows, class Epilogue>
static void launch_wgrad(const typename Rows::Args& a, int NT, hipStream_t s) {
  const dim3 grid(a.Fp / PR_UF, (NT + PR_UN - 1) / PR_UN);
  hipLaunchKernelGGL((k_linear_wgrad<Rows, Epilogue>), grid, dim3(256), 0, s, a);
  HIP_CHECK_LAUNCH();
}

void probe_forward(const ProbeFwdArgs& a, hipStream_t s) {
  if (a.dlT != nullptr) launch_ce_fwd<SweepRows<true>>(a, a.G, s);
  else launch_ce_fwd<SweepRows<false>>(a, a.G, s);
}

void probe_update(const ProbeUpdArgs& a, hipStream_t s) {
  launch_wgrad<GatherRows, SgdEpilogue>(a, a.G * a.Cp, s);
}

void online_probe_forward(const OnlineProbeFwdArgs& a, hipStream_t s) {
  launch_ce_fwd<OnlineRows>(a, 1, s);
}

void online_probe_metrics(const float* loss, const int* rank, int rows, int top_k,
                          double* acc_loss, long long* acc_cnt, hipStream_t s) {
  hipLaunchKernelGGL(k_oprobe_metrics, dim3(1), dim3(256), 0, s, loss, rank, rows, top_k, acc_loss,
                     acc_cnt);
  HIP_CHECK_LAUNCH();
}

void online_probe_wgrad(const OnlineProbeGradArgs& a, hipStream_t s) {
  launch_wgrad<DirectRows, StoreEpilogue>(a, a.Cp, s);
}

void online_probe_update(const OnlineProbeUpdArgs& a, hipStream_t s) {
  const int total = a.Cp * a.Fp + a.Cp;
  hipLaunchKernelGGL(k_oprobe_update, dim3((total + 255) / 256), dim3(256), 0, s, a);
  HIP_CHECK_LAUNCH();
}
