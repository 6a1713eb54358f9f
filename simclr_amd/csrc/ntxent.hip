// Fused NT-Xent (normalised temperature-scaled cross entropy) on gfx950, exact fp32 via the
// f32-input MFMA v_mfma_f32_16x16x4_f32 (cdna_hip_programming.md §3 'FP32-input MFMA').
//
// Reference: /root/reference/loss.py:33-65 — L2-normalise both views, three N×N GEMMs, two
// boolean-mask copies, two concats and two cross-entropies.  Mathematically
// (verified in SURVEY) that is the textbook NT-Xent over 2N anchors: for anchor i the logits are
// s_ij = ẑ_i·ẑ_j / τ over all j ≠ i, the target is the other view of the same image.
//
// Here the similarity matrix is never materialised:
//   fwd   : per 16-anchor tile × column split, S tiles on MFMA, online log-sum-exp, the positive
//           logit picked in-register; a finish kernel merges the splits -> per-row LSE, loss.
//   bwd   : dS = g·(softmax − onehot(pos)) recomputed tile by tile and immediately contracted with
//           the other side's ẑ on MFMA ("owned"/"partner" formulation: the row pass gives
//           Σ_j dS_ij ẑ_j, the column pass Σ_i dS_ij ẑ_i), splits summed by a reduce kernel,
//           then the normalisation backward.
// Columns may be the local rows (reference semantics) or an all-gather of every rank's ẑ
// (``loss.gather``): rows are then columns [col_offset, col_offset+R) of the gathered set.
//
// Data: zn [Ccols][D] fp32 row-major and znT [D][Ccols] fp32 (both produced by the normalise /
// transpose kernels), D % 4 == 0, D <= 256; R % 16 == 0, Ccols % 16 == 0.
#include "common.h"
#include "contrast.h"
#include "kernels.h"

namespace {

typedef float f32x4_t __attribute__((ext_vector_type(4)));

__device__ __forceinline__ int pos_col(int r_local, int n_local, int col_offset) {
  return col_offset + (r_local < n_local ? r_local + n_local : r_local - n_local);
}

// z [R][D] bf16 -> zn [R][D] fp32 normalised, inv_norm [R]; one wave per row
__global__ void k_normalize(const uint16_t* __restrict__ z, int R, int D, float* __restrict__ zn,
                            float* __restrict__ inv_norm) {
  const int row = blockIdx.x * (blockDim.x / 64) + threadIdx.x / 64;
  const int lane = threadIdx.x & 63;
  if (row >= R) return;
  float ss = 0.f;
  for (int d = lane; d < D; d += 64) {
    const float v = bf2f(z[(size_t)row * D + d]);
    ss += v * v;
  }
  ss = wave_sum(ss);
  const float nrm = sqrtf(ss);
  const float inv = 1.f / fmaxf(nrm, 1e-12f);  // F.normalize eps
  for (int d = lane; d < D; d += 64) zn[(size_t)row * D + d] = bf2f(z[(size_t)row * D + d]) * inv;
  if (lane == 0) inv_norm[row] = inv;
}

// in [R][D] -> out [D][ldo] at columns [c0, c0 + R)
__global__ void k_transpose(const float* __restrict__ in, float* __restrict__ out, int R, int D,
                            int ldo, int c0) {
  __shared__ float t[32][33];
  const int r0 = blockIdx.x * 32, d0 = blockIdx.y * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 256 threads: ty 0..7
  for (int k = ty; k < 32; k += 8) {
    const int r = r0 + k, d = d0 + tx;
    t[k][tx] = (r < R && d < D) ? in[(size_t)r * D + d] : 0.f;
  }
  __syncthreads();
  for (int k = ty; k < 32; k += 8) {
    const int d = d0 + k, r = r0 + tx;
    if (d < D && r < R) out[(size_t)d * ldo + c0 + r] = t[tx][k];
  }
}

// S^T tile [partner q (16)][owned o (16)] = Σ_k Z[q][k] Z[o][k]; lane gets (q = 4g+i, o = li)
template <int D>
__device__ __forceinline__ f32x4_t sim_tile(const float* __restrict__ znT, int Ccols, int q0,
                                            const float* breg) {
  const int lane = threadIdx.x & 63;
  const int g = lane >> 4, li = lane & 15;
  f32x4_t a0 = {0.f, 0.f, 0.f, 0.f}, a1 = {0.f, 0.f, 0.f, 0.f};
  constexpr int ksteps = D / 4;
#pragma unroll
  for (int ks = 0; ks < ksteps; ks += 2) {
    const float aq0 = znT[(size_t)(4 * ks + g) * Ccols + q0 + li];
    const float aq1 = znT[(size_t)(4 * (ks + 1) + g) * Ccols + q0 + li];
    a0 = __builtin_amdgcn_mfma_f32_16x16x4f32(aq0, breg[ks], a0, 0, 0, 0);
    a1 = __builtin_amdgcn_mfma_f32_16x16x4f32(aq1, breg[ks + 1], a1, 0, 0, 0);
  }
  return a0 + a1;
}

// ---------------------------------------------------------------- positive rules
// Which columns are an anchor's positives is a compile-time "positive rule"; the forward, finish
// and backward kernels below are written once over it.
//   pair  (NT-Xent): the other view of the anchor's image, pos_col.  Forward partial
//         part[split][r][3] = (max, sumexp, positive logit or -inf); backward weight 1.
//   label (SupCon):  every column but the anchor's own with the anchor's label,
//         loss_i = LSE_{a≠i} s_ia − (1/|P(i)|) Σ_{p∈P(i)} s_ip.  Labels: ycol int32, one per
//         column (view-expanded, rank-major as the columns).  Forward partial
//         part[split][r][4] = (max, sumexp, Σ s over matches, count of matches); backward weight
//         1/|P(anchor)|.
// What the template guarantees: a rule is resolved when the kernel is instantiated, so the pair
// kernels hold no label load, compare or pointer read, and every instantiation runs the same
// online log-sum-exp (contrast.h), the same similarity tiles and the same merge order over lane
// groups and then splits.  With all labels distinct the label rule's arithmetic is therefore
// that of the pair rule operation for operation (one match: the positive sum is that one value
// plus zeros, the count 1.0f, 1/count 1.0f), and the two losses agree bit for bit.

// labels of the four consecutive items [i, i + 4), i % 4 == 0; one 16-byte load if VEC (the
// host picks VEC = the array is 16-byte aligned; compile-time, so the tile loop stays free of
// control flow)
template <bool VEC>
__device__ __forceinline__ void load_labels4(const int* __restrict__ y, int i, int out[4]) {
  if (VEC) {
    const int4 v = *reinterpret_cast<const int4*>(y + i);
    out[0] = v.x, out[1] = v.y, out[2] = v.z, out[3] = v.w;
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) out[k] = y[i + k];
  }
}

// the positive of a row: one logit; lane groups and splits merge by max (-inf where absent)
struct PairPos {
  static constexpr int NP = 3;  // floats per row of a forward partial
  float s = -INFINITY;
  __device__ __forceinline__ void add(float v) { s = v; }
  __device__ __forceinline__ void merge_lanes(int off) { s = fmaxf(s, __shfl_xor(s, off, 64)); }
  __device__ __forceinline__ void merge_split(const float* p) { s = fmaxf(s, p[0]); }
  __device__ __forceinline__ void store(float* p) const { p[0] = s; }
  __device__ __forceinline__ float term(float*, int) const { return s; }
};

// the positives of a row: sum and count, merged by + in lane-group and then split order
struct LabelPos {
  static constexpr int NP = 4;
  float sum = 0.f, cnt = 0.f;
  __device__ __forceinline__ void add(float v) { sum += v, cnt += 1.f; }
  __device__ __forceinline__ void merge_lanes(int off) {
    sum += __shfl_xor(sum, off, 64);
    cnt += __shfl_xor(cnt, off, 64);
  }
  __device__ __forceinline__ void merge_split(const float* p) { sum += p[0], cnt += p[1]; }
  __device__ __forceinline__ void store(float* p) const { p[0] = sum, p[1] = cnt; }
  // mean positive logit; 1/|P| is kept for the backward
  __device__ __forceinline__ float term(float* inv_cnt, int r) const {
    const float ic = 1.f / cnt;
    inv_cnt[r] = ic;
    return sum * ic;
  }
};

// A rule is built per lane from the kernel's arguments and the lane's owned column own_c; r is
// an anchor (local row), c a column, i the partner's place in the lane's four of the tile.
struct PairRule {
  using Pos = PairPos;
  const int n_local, col_offset;
  __device__ __forceinline__ PairRule(const int*, int, const float*, int n_local, int col_offset,
                                      int)
      : n_local(n_local), col_offset(col_offset) {}
  __device__ __forceinline__ void load_tile(int) {}
  __device__ __forceinline__ bool is_pos(int r, int c, bool, int) const {
    return c == pos_col(r, n_local, col_offset);
  }
  __device__ __forceinline__ float pos_weight(int) const { return 1.f; }
};

// ycol holds the labels of the columns [y0, ...); inv_cnt (backward) 1/|P| per local row
template <bool VEC>
struct LabelRule {
  using Pos = LabelPos;
  const int* __restrict__ const ycol;
  const float* __restrict__ const inv_cnt;
  const int y0, y_own;
  int yl[4];
  __device__ __forceinline__ LabelRule(const int* __restrict__ ycol, int y0,
                                       const float* __restrict__ inv_cnt, int, int, int own_c)
      : ycol(ycol), inv_cnt(inv_cnt), y0(y0), y_own(ycol[own_c - y0]) {}
  // the labels of the partner columns [c, c + 4)
  __device__ __forceinline__ void load_tile(int c) { load_labels4<VEC>(ycol, c - y0, yl); }
  __device__ __forceinline__ bool is_pos(int, int, bool self, int i) const {
    return !self & (yl[i] == y_own);
  }
  __device__ __forceinline__ float pos_weight(int r) const { return inv_cnt[r]; }
};

// ---------------------------------------------------------------- negative rules
// How the other columns enter an anchor's denominator is a compile-time "negative rule", the
// second axis of the same kernels.
//   plain    (NT-Xent, SupCon): every column but the anchor's own, the positives included, in one
//            log-sum-exp; backward weight exp(s − lse).  This is the code as it was: the rule has
//            no state and no kernel argument, and the kernels branch on it with `if constexpr`.
//   weighted (pair rule only; hard-negative / debiased / decoupled NT-Xent, loss/ntxent.py): the
//            positive is kept out of the sums and carried as s_ip; L1 = LSE_Neg (1+β)s and, for
//            HARD (β > 0), L0 = LSE_Neg βs in a second online log-sum-exp of the same helpers
//            (HARD = false: L0 = log N, no second sum, no second exp, no argument).  Forward
//            partial part[split][r][3 or 5] = (m1, l1, s_ip or -inf[, m0, l0]).  The finish kernel
//            evaluates the shifted form per row and leaves stats[r] = (L1, A, B, L0); backward
//            weight A·((1+β)·exp((1+β)s − L1) − β·exp(βs − L0)) at a negative, B at the positive.
struct PlainNeg {
  static constexpr bool WEIGHTED = false;
  static constexpr int NX = 0;  // floats per row of a forward partial beyond Pos::NP
};

template <bool HARD_>
struct WeightedNeg {
  static constexpr bool WEIGHTED = true, HARD = HARD_;
  static constexpr int NX = HARD ? 2 : 0;
  const float beta, beta1;  // β, 1 + β
  float m0 = -INFINITY, l0 = 0.f;
  // the kernels' trailing arguments: β for HARD, none otherwise
  __device__ __forceinline__ WeightedNeg() : beta(0.f), beta1(1.f) {}
  __device__ __forceinline__ explicit WeightedNeg(float beta) : beta(beta), beta1(1.f + beta) {}
  __device__ __forceinline__ void push(float& m, float& l, float v) {
    if (HARD) {
      lse_push(m, l, beta1 * v);
      lse_push(m0, l0, beta * v);
    } else {
      lse_push(m, l, v);
    }
  }
  __device__ __forceinline__ void merge_lanes(int off) {
    if (HARD) lse_merge_lanes(m0, l0, off);
  }
  __device__ __forceinline__ void store(float* p) const {
    if (HARD) p[0] = m0, p[1] = l0;
  }
  // dS_ia / (g·A_i) at a negative with logit v, st = (L1, A, B, L0) of the anchor
  __device__ __forceinline__ float neg_weight(float v, const float4& st) const {
    if (HARD) return beta1 * __expf(beta1 * v - st.x) - beta * __expf(beta * v - st.w);
    return __expf(v - st.x);
  }
};

// Forward: grid (R/16, splits), one wave per block. Owned = anchor rows [r0, r0+16) (local),
// partners = columns [c_beg, c_end). Writes part[split][r][Pos::NP + Neg::NX], self excluded.
// ycol / y0 are the label rule's (the window and the owned rows lie inside), n_local the pair
// rule's, neg_args the negative rule's (none for the plain rule).
template <int D, class Rule, class Neg = PlainNeg, class... NegArgs>
__global__ __launch_bounds__(64) void k_ntxent_fwd(const float* __restrict__ znT,
                                                     int R, int Ccols, int col_offset,
                                                     int n_local, float inv_temp,
                                                     int cols_per_split, float* __restrict__ part,
                                                     int c_lo, int c_hi, int split_base,
                                                     const int* __restrict__ ycol, int y0,
                                                     NegArgs... neg_args) {
  const int lane = threadIdx.x;
  const int g = lane >> 4, li = lane & 15;
  const int r0 = blockIdx.x * 16;
  const int split = split_base + blockIdx.y;
  const int c_beg = c_lo + blockIdx.y * cols_per_split;
  int c_end = c_beg + cols_per_split;
  if (c_end > c_hi) c_end = c_hi;
  float breg[D / 4];
#pragma unroll
  for (int ks = 0; ks < D / 4; ++ks)
    breg[ks] = znT[(size_t)(4 * ks + g) * Ccols + col_offset + r0 + li];
  const int my_r = r0 + li;  // owned row of this lane (o = li)
  const int self_c = col_offset + my_r;
  Rule rule(ycol, y0, nullptr, n_local, col_offset, self_c);
  typename Rule::Pos pos;
  [[maybe_unused]] Neg neg{neg_args...};
  float m = -INFINITY, l = 0.f;
  for (int q0 = c_beg; q0 < c_end; q0 += 16) {
    const f32x4_t s = sim_tile<D>(znT, Ccols, q0, breg);
    rule.load_tile(q0 + 4 * g);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int c = q0 + 4 * g + i;
      const float v = s[i] * inv_temp;
      const bool self = c == self_c;
      if constexpr (Neg::WEIGHTED) {
        const bool p = rule.is_pos(my_r, c, self, i);
        if (p) pos.add(v);
        if (!(self | p)) neg.push(m, l, v);
      } else {
        if (rule.is_pos(my_r, c, self, i)) pos.add(v);
        if (!self) lse_push(m, l, v);
      }
    }
  }
  // merge across the 4 lane groups (g) holding the same row
#pragma unroll
  for (int off = 16; off < 64; off <<= 1) {
    lse_merge_lanes(m, l, off);
    pos.merge_lanes(off);
    if constexpr (Neg::WEIGHTED) neg.merge_lanes(off);
  }
  if (g == 0) {
    float* dst = part + ((size_t)split * R + my_r) * (Rule::Pos::NP + Neg::NX);
    dst[0] = m;
    dst[1] = l;
    pos.store(dst + 2);
    if constexpr (Neg::WEIGHTED) neg.store(dst + Rule::Pos::NP);
  }
}

// The weighted rule's finish: merge splits in order, then per row, with N = the number of
// negatives, u = L1 − L0, c = max(u, s_ip) (every exp argument below is <= 0):
//   raw = N·(e^{u−c} − τ⁺·e^{s_ip−c}) / (1 − τ⁺),  floor = N·e^{−1/τ−c},  k = [raw >= floor],
//   T = κ·e^{s_ip−c} + max(raw, floor),  loss = −s_ip + c + log T,
//   A = k·N/(1−τ⁺)·e^{u−c}/T,  B = −1 + (κ − k·τ⁺·N/(1−τ⁺))·e^{s_ip−c}/T.
// stats[r] = (L1, A, B, L0) for the backward passes.
template <bool HARD>
__global__ void k_ntxent_finish_weighted(const float* __restrict__ part, int R, int splits,
                                         float nneg, float inv_temp, float tau_plus, float kappa,
                                         float4* __restrict__ stats, float* __restrict__ loss) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= R) return;
  constexpr int NP = PairPos::NP + WeightedNeg<HARD>::NX;
  float m = -INFINITY, l = 0.f, m0 = -INFINITY, l0 = 0.f;
  PairPos pos;
  for (int s = 0; s < splits; ++s) {
    const float* p = part + ((size_t)s * R + r) * NP;
    lse_merge_split(m, l, p);
    pos.merge_split(p + 2);
    if (HARD) lse_merge_split(m0, l0, p + PairPos::NP);
  }
  const float L1 = m + logf(l);
  const float L0 = HARD ? m0 + logf(l0) : logf(nneg);
  const float sp = pos.s;
  const float u = L1 - L0;
  const float c = fmaxf(u, sp);
  const float eu = expf(u - c), ep = expf(sp - c);
  const float q = nneg / (1.f - tau_plus);
  const float raw = q * (eu - tau_plus * ep);
  const float floor_ = nneg * expf(-inv_temp - c);
  const bool k = raw >= floor_;
  const float T = kappa * ep + fmaxf(raw, floor_);
  // a clamped row has c = s_ip; decoupled (T = floor) its floor can underflow at a small
  // temperature, where log T = log N − 1/τ − c is known and A = 0, B = −1 exactly
  const float log_T = (!k && kappa == 0.f) ? logf(nneg) - inv_temp - c : logf(T);
  loss[r] = -sp + c + log_T;
  // B in the contract's form, the one the twin's autograd takes (a clamped row with κ = 1 has
  // B = −floor/T of the order of its loss, by cancellation in fp32 on both sides)
  const float cb = kappa - (k ? tau_plus * q : 0.f);
  const float B = (cb != 0.f && T > 0.f) ? -1.f + cb * ep / T : -1.f;
  stats[r] = make_float4(L1, (k && T > 0.f) ? q * eu / T : 0.f, B, L0);
}

// merge splits in order -> lse[r], loss[r] (and the label rule's inv_cnt[r] = 1/|P(r)|)
template <class Pos>
__global__ void k_ntxent_finish(const float* __restrict__ part, int R, int splits,
                                  float* __restrict__ lse, float* __restrict__ inv_cnt,
                                  float* __restrict__ loss) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= R) return;
  float m = -INFINITY, l = 0.f;
  Pos pos;
  for (int s = 0; s < splits; ++s) {
    const float* p = part + ((size_t)s * R + r) * Pos::NP;
    lse_merge_split(m, l, p);
    pos.merge_split(p + 2);
  }
  const float ls = m + logf(l);
  lse[r] = ls;
  loss[r] = ls - pos.term(inv_cnt, r);
}

// Backward (owned/partner). ROW mode: owned = local anchor rows (lse by owned), partners =
// columns. COL mode: owned = columns [o0..), partners = local anchor rows (lse by partner).
// out[split][owned][D] += Σ_q w(q,o) ẑ_q ;
// w = gscale·(exp(s−lse_anchor) − [col∈P(anchor)]·pos_weight(anchor)); ycol covers every column.
// Weighted rule: lse holds the finish kernel's stats, (L1, A, B, L0) per local row, and
// w = gscale·(B_anchor at the positive, A_anchor·neg_weight at a negative, 0 at the anchor's own).
template <bool ROW, int D, class Rule, class Neg = PlainNeg, class... NegArgs>
__global__ __launch_bounds__(64) void k_ntxent_bwd(const float* __restrict__ zn,
                                                     const float* __restrict__ znT,
                                                     const float* __restrict__ lse, int R,
                                                     int Ccols, int col_offset, int n_local,
                                                     float inv_temp, float gscale,
                                                     const float* __restrict__ gout,
                                                     int partners_per_split,
                                                     float* __restrict__ out,
                                                     const float* __restrict__ inv_cnt,
                                                     const int* __restrict__ ycol,
                                                     NegArgs... neg_args) {
  const int lane = threadIdx.x;
  const int g = lane >> 4, li = lane & 15;
  const int o0 = blockIdx.x * 16;  // ROW: local row index; COL: column index
  const int split = blockIdx.y;
  const int nown = ROW ? R : Ccols;
  const int npart = ROW ? Ccols : R;
  const int q_beg = split * partners_per_split;
  int q_end = q_beg + partners_per_split;
  if (q_end > npart) q_end = npart;
  const float gs = gscale * (gout ? gout[0] : 1.f);
  // owned operand (B of the similarity MFMA): column index in znT of owned item li
  const int own_col = ROW ? (col_offset + o0 + li) : (o0 + li);
  float breg[D / 4];
#pragma unroll
  for (int ks = 0; ks < D / 4; ++ks) breg[ks] = znT[(size_t)(4 * ks + g) * Ccols + own_col];
  Rule rule(ycol, 0, inv_cnt, n_local, col_offset, own_col);
  [[maybe_unused]] const Neg neg{neg_args...};
  [[maybe_unused]] const float4* __restrict__ const stats = reinterpret_cast<const float4*>(lse);
  float lse_own = 0.f, pw_own = 0.f;
  [[maybe_unused]] float4 st_own = {0.f, 0.f, 0.f, 0.f};
  if (ROW) {
    if constexpr (Neg::WEIGHTED) {
      st_own = stats[o0 + li];
    } else {
      lse_own = lse[o0 + li];
      pw_own = rule.pos_weight(o0 + li);
    }
  }
  constexpr int nd = D / 16;
  f32x4_t acc[nd];
#pragma unroll
  for (int t = 0; t < nd; ++t) acc[t] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
  for (int q0 = q_beg; q0 < q_end; q0 += 16) {
    const int qcol0 = ROW ? q0 : (col_offset + q0);  // partner column index in znT / zn
    const f32x4_t s = sim_tile<D>(znT, Ccols, qcol0, breg);
    rule.load_tile(qcol0 + 4 * g);  // (ROW: columns; COL: anchors, as columns of this rank)
    float w[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float v = s[i] * inv_temp;
      const int r = ROW ? o0 + li : q0 + 4 * g + i;  // anchor (local row)
      const int c = ROW ? q0 + 4 * g + i : o0 + li;  // column
      if constexpr (Neg::WEIGHTED) {
        const float4 sa = ROW ? st_own : stats[r];  // (loaded unconditionally, as lse below)
        const bool self = c == col_offset + r;
        const bool pos = rule.is_pos(r, c, self, i);
        const float p = sa.y * neg.neg_weight(v, sa);
        w[i] = gs * (self ? 0.f : (pos ? sa.z : p));
      } else {
        const float la = ROW ? lse_own : lse[r];
        const bool self = c == col_offset + r;
        const bool pos = rule.is_pos(r, c, self, i);
        const float p = self ? 0.f : __expf(v - la);
        w[i] = gs * (p - (pos ? (ROW ? pw_own : rule.pos_weight(r)) : 0.f));
      }
    }
    // acc[o][d] += Σ_q w(q,o) Z[q][d]: A[o=li][k=g] = w[t] (q = 4g+t), B[k=g][d=li] = Z[q][d]
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const float* zrow = zn + (size_t)(qcol0 + 4 * g + t) * D + li;
#pragma unroll
      for (int dt = 0; dt < nd; ++dt)
        acc[dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[t], zrow[dt * 16], acc[dt], 0, 0, 0);
    }
  }
  // lane holds out[o = 4g+i][d = dt*16 + li]
  float* dst = out + (size_t)split * nown * D;
#pragma unroll
  for (int dt = 0; dt < nd; ++dt)
#pragma unroll
    for (int i = 0; i < 4; ++i)
      dst[(size_t)(o0 + 4 * g + i) * D + dt * 16 + li] = acc[dt][i] * inv_temp;
}

// The rank's label block: out[v·n + i] = labels[idx ? idx[i] : i] for every view v, as int32.
// (idx: the batch's index vector into the dataset's labels; an index outside [0, n_src) is
// clamped into it, so a bad index cannot read outside the array.)
template <typename T>
__global__ void k_expand_labels(const T* __restrict__ labels, const int64_t* __restrict__ idx,
                                long n_src, int n, int views, int* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  long j = idx ? (long)idx[i] : (long)i;
  j = j < 0 ? 0 : (j >= n_src ? n_src - 1 : j);
  const int y = (int)labels[j];
  for (int v = 0; v < views; ++v) out[(size_t)v * n + i] = y;
}

// out[r][d] = Σ_s part[s][r][d]   (n elems per split)
__global__ void k_sum_splits(const float* __restrict__ part, int splits, size_t n,
                             float* __restrict__ out) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (size_t)gridDim.x * blockDim.x) {
    float s = 0.f;
    for (int k = 0; k < splits; ++k) s += part[(size_t)k * n + i];
    out[i] = s;
  }
}

// dz = (dẑ − ẑ (ẑ·dẑ)) · inv_norm ; one wave per row
__global__ void k_normalize_bwd(const float* __restrict__ zn, const float* __restrict__ inv_norm,
                                const float* __restrict__ dzn, int R, int D,
                                uint16_t* __restrict__ dz_bf16, float* __restrict__ dz_f32) {
  const int row = blockIdx.x * (blockDim.x / 64) + threadIdx.x / 64;
  const int lane = threadIdx.x & 63;
  if (row >= R) return;
  float dot = 0.f;
  for (int d = lane; d < D; d += 64) dot += zn[(size_t)row * D + d] * dzn[(size_t)row * D + d];
  dot = wave_sum(dot);
  const float inv = inv_norm[row];
  for (int d = lane; d < D; d += 64) {
    const size_t i = (size_t)row * D + d;
    const float v = (dzn[i] - zn[i] * dot) * inv;
    if (dz_bf16) dz_bf16[i] = f2bf(v);
    if (dz_f32) dz_f32[i] = v;
  }
}

__global__ void k_reduce_loss(const float* __restrict__ loss, int R, float scale,
                              float* __restrict__ out) {
  __shared__ float red[16];
  float s = 0.f;
  for (int i = threadIdx.x; i < R; i += blockDim.x) s += loss[i];
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    float t = 0.f;
    for (int w = 0; w < (int)(blockDim.x >> 6); ++w) t += red[w];
    out[0] = t * scale;
  }
}

// One-wave blocks, latency-bound on their L2 operand loads: each block should walk about 8
// partner tiles (128 columns), with at least 512 blocks (so the SIMDs have waves to switch
// between) and at most 4096 (the split partials grow with the count).  tools/ntxent_bench.py,
// R = 1024: at 8192 global negatives (8 ranks) the fixed 512-block rule took 85 + 107 + 327 µs
// (forward, column and row gradient passes), this one ~57 + 78 + 94; at 1024 columns it keeps
// 512.
int splits_for(int tiles, int ptiles, int tiles_per_block = 8) {
  long target = (long)tiles * ptiles / tiles_per_block;
  target = target < 512 ? 512 : (target > 4096 ? 4096 : target);
  int s = (int)((target + tiles - 1) / tiles);
  if (s > ptiles) s = ptiles;
  if (s < 1) s = 1;
  return s;
}

}  // namespace

// ------------------------------------------------------------------- host API (raw pointers)
void ntxent_normalize_f32(const uint16_t* z, int R, int D, float* zn, float* inv_norm,
                          hipStream_t s) {
  hipLaunchKernelGGL(k_normalize, dim3((R + 3) / 4), dim3(256), 0, s, z, R, D, zn, inv_norm);
  HIP_CHECK_LAUNCH();
}

void ntxent_transpose_cols(const float* in, float* out, int R, int D, int ldo, int c0,
                           hipStream_t s) {
  hipLaunchKernelGGL(k_transpose, dim3((R + 31) / 32, (D + 31) / 32), dim3(256), 0, s, in, out, R,
                     D, ldo, c0);
  HIP_CHECK_LAUNCH();
}

void ntxent_transpose(const float* in, float* out, int R, int D, hipStream_t s) {
  ntxent_transpose_cols(in, out, R, D, R, 0, s);
}

// measured optimum (tools/ntxent_bench.py, 8192 columns): ~16 partner tiles per block for the
// forward (57 µs vs 74 at 8) and the column pass (73 vs 78), ~8 for the row pass (93 vs 110)
int ntxent_fwd_splits(int R, int Ccols) { return splits_for(R / 16, Ccols / 16, 16); }
int ntxent_bwd_splits(int nown, int npart) {
  return splits_for(nown / 16, npart / 16, nown <= npart ? 8 : 16);
}

static bool labels_vec(const int* y) { return ((uintptr_t)y & 15) == 0; }

// Runs the statement(s) with RULE = the positive rule: the label rule if there are labels (its
// 16-byte loads if they are aligned), else the pair rule.
#define DISPATCH_RULE(ycol, ...)                                            \
  if (!(ycol)) { using RULE = PairRule; __VA_ARGS__; }                      \
  else if (labels_vec(ycol)) { using RULE = LabelRule<true>; __VA_ARGS__; } \
  else { using RULE = LabelRule<false>; __VA_ARGS__; }

// columns [c_lo, c_hi) of znT into splits [split_base, split_base + splits) of part
// (y0 % 16 == 0: the tile offsets keep the labels' alignment)
static void forward_range(const float* znT, const int* ycol, int y0, int R, int Ccols, int D,
                          int col_offset, int n_local, float inv_temp, float* part, int c_lo,
                          int c_hi, int splits, int split_base, hipStream_t s) {
  const int ptiles = (c_hi - c_lo) / 16;
  const int per = ((ptiles + splits - 1) / splits) * 16;
  DISPATCH_D(D, "ntxent", DISPATCH_RULE(ycol, hipLaunchKernelGGL(
      (k_ntxent_fwd<DD, RULE>), dim3(R / 16, splits), dim3(64), 0, s, znT, R, Ccols, col_offset,
      n_local, inv_temp, per, part, c_lo, c_hi, split_base, ycol, y0)));
  HIP_CHECK_LAUNCH();
}

// out[i] = Σ_k part[k][i], i < n
static void sum_splits(const float* part, int splits, size_t n, float* out, hipStream_t s) {
  int blocks = (int)((n + 255) / 256);
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(k_sum_splits, dim3(blocks), dim3(256), 0, s, part, splits, n, out);
  HIP_CHECK_LAUNCH();
}

static void backward_part(int row_mode, const float* zn, const float* znT, const float* lse,
                          const float* inv_cnt, const int* ycol, int R, int Ccols, int D,
                          int col_offset, int n_local, float inv_temp, float gscale,
                          const float* gout, float* part, int splits, float* out, hipStream_t s) {
  const int nown = row_mode ? R : Ccols;
  const int npart = row_mode ? Ccols : R;
  const int ptiles = npart / 16;
  const int per = ((ptiles + splits - 1) / splits) * 16;
#define BWD_LAUNCH(ROW)                                                                         \
  hipLaunchKernelGGL((k_ntxent_bwd<ROW, DD, RULE>), dim3(nown / 16, splits), dim3(64), 0, s,  \
                     zn, znT, lse, R, Ccols, col_offset, n_local, inv_temp, gscale, gout, per,  \
                     part, inv_cnt, ycol)
  DISPATCH_D(D, "ntxent", DISPATCH_RULE(ycol, if (row_mode) BWD_LAUNCH(true);
                                        else BWD_LAUNCH(false)));
#undef BWD_LAUNCH
  HIP_CHECK_LAUNCH();
  sum_splits(part, splits, (size_t)nown * D, out, s);
}

void ntxent_forward_range(const float* znT, int R, int Ccols, int D, int col_offset, int n_local,
                          float inv_temp, float* part, int c_lo, int c_hi, int splits,
                          int split_base, hipStream_t s) {
  forward_range(znT, nullptr, 0, R, Ccols, D, col_offset, n_local, inv_temp, part, c_lo, c_hi,
                splits, split_base, s);
}

void ntxent_finish(const float* part, int R, int splits, float* lse, float* loss, hipStream_t s) {
  hipLaunchKernelGGL(k_ntxent_finish<PairPos>, dim3((R + 255) / 256), dim3(256), 0, s, part, R,
                     splits, lse, nullptr, loss);
  HIP_CHECK_LAUNCH();
}

void ntxent_forward(const float* znT, int R, int Ccols, int D, int col_offset, int n_local,
                    float inv_temp, float* part, int splits, float* lse, float* loss,
                    hipStream_t s) {
  ntxent_forward_range(znT, R, Ccols, D, col_offset, n_local, inv_temp, part, 0, Ccols, splits, 0,
                       s);
  ntxent_finish(part, R, splits, lse, loss, s);
}

void ntxent_backward_part(int row_mode, const float* zn, const float* znT, const float* lse, int R,
                          int Ccols, int D, int col_offset, int n_local, float inv_temp,
                          float gscale, const float* gout, float* part, int splits, float* out,
                          hipStream_t s) {
  backward_part(row_mode, zn, znT, lse, nullptr, nullptr, R, Ccols, D, col_offset, n_local,
                inv_temp, gscale, gout, part, splits, out, s);
}

// ---- weighted negatives (pair rule; hard-negative / debiased / decoupled NT-Xent): beta > 0
// picks WeightedNeg<true> and its 5-float partials, beta == 0 WeightedNeg<false> (3 floats)
void ntxent_weighted_forward_range(const float* znT, int R, int Ccols, int D, int col_offset,
                                   int n_local, float inv_temp, float beta, float* part, int c_lo,
                                   int c_hi, int splits, int split_base, hipStream_t s) {
  const int ptiles = (c_hi - c_lo) / 16;
  const int per = ((ptiles + splits - 1) / splits) * 16;
#define WFWD_LAUNCH(HARD, ...)                                                                   \
  hipLaunchKernelGGL((k_ntxent_fwd<DD, PairRule, WeightedNeg<HARD>>), dim3(R / 16, splits),     \
                     dim3(64), 0, s, znT, R, Ccols, col_offset, n_local, inv_temp, per, part,    \
                     c_lo, c_hi, split_base, (const int*)nullptr, 0, ##__VA_ARGS__)
  DISPATCH_D(D, "ntxent", if (beta > 0.f) WFWD_LAUNCH(true, beta); else WFWD_LAUNCH(false));
#undef WFWD_LAUNCH
  HIP_CHECK_LAUNCH();
}

void ntxent_weighted_finish(const float* part, int R, int splits, int Ccols, float inv_temp,
                            float beta, float tau_plus, int decoupled, float* stats, float* loss,
                            hipStream_t s) {
  const float nneg = (float)(Ccols - 2), kappa = decoupled ? 0.f : 1.f;
  const dim3 grid((R + 255) / 256), block(256);
  if (beta > 0.f)
    hipLaunchKernelGGL(k_ntxent_finish_weighted<true>, grid, block, 0, s, part, R, splits, nneg,
                       inv_temp, tau_plus, kappa, (float4*)stats, loss);
  else
    hipLaunchKernelGGL(k_ntxent_finish_weighted<false>, grid, block, 0, s, part, R, splits, nneg,
                       inv_temp, tau_plus, kappa, (float4*)stats, loss);
  HIP_CHECK_LAUNCH();
}

void ntxent_weighted_backward_part(int row_mode, const float* zn, const float* znT,
                                   const float* stats, int R, int Ccols, int D, int col_offset,
                                   int n_local, float inv_temp, float beta, float gscale,
                                   const float* gout, float* part, int splits, float* out,
                                   hipStream_t s) {
  const int nown = row_mode ? R : Ccols;
  const int npart = row_mode ? Ccols : R;
  const int ptiles = npart / 16;
  const int per = ((ptiles + splits - 1) / splits) * 16;
#define WBWD_LAUNCH(ROW, HARD, ...)                                                              \
  hipLaunchKernelGGL((k_ntxent_bwd<ROW, DD, PairRule, WeightedNeg<HARD>>),                      \
                     dim3(nown / 16, splits), dim3(64), 0, s, zn, znT, stats, R, Ccols,          \
                     col_offset, n_local, inv_temp, gscale, gout, per, part,                     \
                     (const float*)nullptr, (const int*)nullptr, ##__VA_ARGS__)
  DISPATCH_D(D, "ntxent",
             if (beta > 0.f) { if (row_mode) WBWD_LAUNCH(true, true, beta);
                               else WBWD_LAUNCH(false, true, beta); }
             else { if (row_mode) WBWD_LAUNCH(true, false); else WBWD_LAUNCH(false, false); });
#undef WBWD_LAUNCH
  HIP_CHECK_LAUNCH();
  sum_splits(part, splits, (size_t)nown * D, out, s);
}

// ---- label mode (SupCon): ycol must not be null (the pair rule needs n_local, which these
// do not take)
void supcon_forward_range(const float* znT, const int* ycol, int y0, int R, int Ccols, int D,
                          int col_offset, float inv_temp, float* part, int c_lo, int c_hi,
                          int splits, int split_base, hipStream_t s) {
  forward_range(znT, ycol, y0, R, Ccols, D, col_offset, 0, inv_temp, part, c_lo, c_hi, splits,
                split_base, s);
}

void supcon_finish(const float* part, int R, int splits, float* lse, float* inv_cnt, float* loss,
                   hipStream_t s) {
  hipLaunchKernelGGL(k_ntxent_finish<LabelPos>, dim3((R + 255) / 256), dim3(256), 0, s, part, R,
                     splits, lse, inv_cnt, loss);
  HIP_CHECK_LAUNCH();
}

void supcon_backward_part(int row_mode, const float* zn, const float* znT, const float* lse,
                          const float* inv_cnt, const int* ycol, int R, int Ccols, int D,
                          int col_offset, float inv_temp, float gscale, const float* gout,
                          float* part, int splits, float* out, hipStream_t s) {
  backward_part(row_mode, zn, znT, lse, inv_cnt, ycol, R, Ccols, D, col_offset, 0, inv_temp,
                gscale, gout, part, splits, out, s);
}

void supcon_expand_labels(const void* labels, int labels_i64, const int64_t* idx, long n_src,
                          int n, int views, int* out, hipStream_t s) {
  const dim3 grid((n + 255) / 256), block(256);
  if (labels_i64)
    hipLaunchKernelGGL(k_expand_labels<int64_t>, grid, block, 0, s, (const int64_t*)labels, idx,
                       n_src, n, views, out);
  else
    hipLaunchKernelGGL(k_expand_labels<int>, grid, block, 0, s, (const int*)labels, idx, n_src, n,
                       views, out);
  HIP_CHECK_LAUNCH();
}

void ntxent_normalize_backward(const float* zn, const float* inv_norm, const float* dzn, int R,
                               int D, uint16_t* dz_bf16, float* dz_f32, hipStream_t s) {
  hipLaunchKernelGGL(k_normalize_bwd, dim3((R + 3) / 4), dim3(256), 0, s, zn, inv_norm, dzn, R, D,
                     dz_bf16, dz_f32);
  HIP_CHECK_LAUNCH();
}

void ntxent_reduce_loss(const float* loss_rows, int R, float scale, float* out, hipStream_t s) {
  hipLaunchKernelGGL(k_reduce_loss, dim3(1), dim3(1024), 0, s, loss_rows, R, scale, out);
  HIP_CHECK_LAUNCH();
}
