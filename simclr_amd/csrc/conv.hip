// Implicit-GEMM convolution engine for gfx950 (MI355X), bf16 NHWC, fp32 accumulation on MFMA.
//
// Replaces the implicit cuDNN/MIOpen convolutions of the reference's torchvision ResNet
// (/root/reference/model.py:76-114).  Two kernels cover all three conv passes:
//
//   igemm_nt  C[M,N] = im2col(A)[M,K] · B[N,K]^T     forward  (B = weight, OHWI)
//                                                    dgrad    (A = dY, B = flipped / parity-class
//                                                              sub-kernel weight, see conv_hip.py)
//             epilogue: + bias, bf16 NHWC store through LDS (16-B row stores, strided output
//             mapping for stride-2 dgrad parity classes) and per-(segment, channel) Σx / Σx²
//             partials for the following BatchNorm (saves the BN statistics read pass).
//   wgrad_tn  dW[N,K] = Σ_m dY[m,N]^T · im2col(X)[m,K] split over m; both operands are staged
//             row-major in LDS and read as MFMA fragments with ds_read_b64_tr_b16 (the transpose
//             is free).  fp32 partial slabs are summed by wgrad_reduce straight into the flat fp32
//             gradient buffer (OHWI = the im2col K order).
//
// Fusions: optional *prologue* applies a per-(segment, channel) affine + ReLU to the gathered A
// operand on its way into LDS (= the previous BatchNorm's normalise+ReLU, so that BN output is
// never written to HBM; conv padding stays exactly zero), and the igemm *epilogue* can accumulate
// a residual (out += r) or a ReLU-masked gradient (out += (y > 0) ? dy : 0) while storing.
// Several tile shapes are instantiated; the host autotunes one per problem shape.
//
// Gather: the A operand is addressed per 16-byte chunk (8 channels) with raw buffer loads whose
// out-of-range offset returns zeros, so conv padding / M and K tails need no branches around the
// loads.  Tiles: BM x BN x 64, 256 threads (4 waves), mfma_f32_16x16x32_bf16, LDS double buffer
// with an XOR chunk swizzle (cdna_hip_programming.md T2), XCD-aware block remap (T1).
#include <cstring>
#include "common.h"
#include "kernels.h"

#include <type_traits>
#include <utility>

namespace {

struct IgemmArgs {
  const uint16_t* A;
  const uint16_t* B;
  uint16_t* out;
  const float* bias;
  float* stats;  // [gridM][2][N] partial Σx, Σx² (bf16-rounded outputs) or nullptr
  int M, N, K;
  int IH, IW, C;
  int OH, OW, KW;
  int ish, isw, dh, dw, ih0, iw0;
  int OHp, OWp, osh, osw, ooh, oow, ldo;
  int direct_out;
  uint32_t a_bytes, b_bytes;
  int nMb, nNb;
  // prologue (A operand): a = relu?(x * sc[seg][c] + sh[seg][c]); seg = m / pro_seg_rows
  // or (pro_d != nullptr) the BatchNorm-backward form a = sc·A + sh·A2 + d (da = A·g + B·x + D
  // of the BN that follows this conv's input in forward order), reading A2 at A's offsets
  const float* pro_sc;
  const float* pro_sh;
  const float* pro_d;
  const uint16_t* A2;
  int pro_seg_rows, pro_relu;
  // block-output prologue (igemm_glds PRO == 3): a = relu(A·sc + sh + (A2·rsc + rsh | A2)) —
  // the previous block's BN3 + downsample BN / identity residual + ReLU — which is also the
  // block output itself: stored to pro_out with its ReLU bitmask pro_mask (see bn_apply_ss)
  const float* pro_rsc;
  const float* pro_rsh;
  uint16_t* pro_out;
  uint8_t* pro_mask;
  // epilogue: 0 store, 1 out = acc + epi_a, 2 out = acc + (epi_b > 0 ? epi_a : 0),
  // 3 out = g = (epi_b*sc + sh > 0) ? acc : 0 with BatchNorm-backward partials Σg, Σg·x̂
  //   (x̂ = (epi_b - mean)·invstd) in place of Σy, Σy² (ReLU mask + BN bwd reduce of the
  //   producing layer, fused into the dgrad that computes its output gradient)
  // 4 v = acc + epi_a; out = g = (epi_b > 0) ? v : 0 with partials Σg, Σg·x̂ (x̂ from epi_c):
  //   the block-input gradient of a residual block, already masked by the previous block's
  //   output ReLU, with that block's last-BN backward reduce folded in
  int epi_mode;
  int epi_a_sub;  // epi_a: stride-2 subsampled residual (direct output only), see ConvFusion
  const uint16_t* epi_a;
  const uint16_t* epi_b;
  const uint16_t* epi_c;
  const uint8_t* epi_mask;  // mode 4: ReLU bitmask (bit e of byte o/8) instead of epi_b
  const uint16_t* epi_c2;   // mode 4: second pre-BN activation (the producer's downsample BN)
  const float* epi_mi2;     //   its mean / invstd [2][S][N]
  float* stats2;            //   its partials Σg, Σg·x̂2 (same row layout as stats)
  const float* epi_ss;  // mode 3: [2][S][N] BN scale / shift
  const float* epi_mi;  // mode 3/4: [2][S][N] BN mean / invstd
  int epi_S;
  // stats row remap (segment-major partials when one BN's rows span several launches):
  //   blk = seg * stats_seg_blocks + stats_base + (m0 - seg * seg_rows) / BM, seg = m0 / seg_rows
  int seg_rows, stats_seg_blocks, stats_base;
};

// Raw buffer resource over [p, p + bytes): offsets at or past `bytes` load zeros (the gathers'
// padding and tail handling rests on that).  0x00020000 = DATA_FORMAT 32 bit, no swizzle.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t buf_rsrc(const void* p, uint32_t bytes) {
  return __builtin_amdgcn_make_buffer_rsrc((void*)p, (short)0, (int)bytes, 0x00020000);
}

__device__ __forceinline__ u32x4 affine_relu8(u32x4 v, const float* sc, const float* sh, bool ok,
                                              bool relu) {
  u32x4 w;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    float a = lo_bf(v[e]) * sc[2 * e] + sh[2 * e];
    float b = hi_bf(v[e]) * sc[2 * e + 1] + sh[2 * e + 1];
    if (relu) {
      a = fmaxf(a, 0.f);
      b = fmaxf(b, 0.f);
    }
    w[e] = ok ? pack2bf(a, b) : 0u;
  }
  return w;
}

// Packed form of affine_relu8 for the register-side prologue (no out-of-range lanes): two
// channels per v_pk_fma_f32, one v_cvt_pk_bf16_f32, and the ReLU as a packed signed 16-bit max
// on the bf16 bit patterns (a negative bf16 is a negative int16; -0 becomes +0)
__device__ __forceinline__ u32x4 affine_relu8_pk(u32x4 v, const f32x2* sc, const f32x2* sh,
                                                 bool relu) {
  typedef short i16x2 __attribute__((ext_vector_type(2)));
  u32x4 w;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const f32x2 x = {lo_bf(v[e]), hi_bf(v[e])};
    const f32x2 y = __builtin_elementwise_fma(x, sc[e], sh[e]);
    uint32_t q = pack2bf(y.x, y.y);
    if (relu)
      q = __builtin_bit_cast(uint32_t, __builtin_elementwise_max(__builtin_bit_cast(i16x2, q),
                                                                 (i16x2){0, 0}));
    w[e] = q;
  }
  return w;
}

__device__ __forceinline__ u32x4 bnbwd8(u32x4 g, u32x4 x, const float* A, const float* B,
                                        const float* D, bool ok) {
  u32x4 w;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const float a = A[2 * e] * lo_bf(g[e]) + B[2 * e] * lo_bf(x[e]) + D[2 * e];
    const float b = A[2 * e + 1] * hi_bf(g[e]) + B[2 * e + 1] * hi_bf(x[e]) + D[2 * e + 1];
    w[e] = ok ? pack2bf(a, b) : 0u;
  }
  return w;
}

// Epilogue row batches: the global operands of UNR output rows (per thread) are loaded together.
template <int BM, int BN, int NT>
constexpr int epi_unr() {
  return (BM / (NT / (BN / 8))) < 4 ? (BM / (NT / (BN / 8))) : 4;
}

template <int UNR>
struct EpiBatch {
  size_t o[UNR];
  bool ok[UNR];
  u32x4 ea[UNR], eb[UNR], ec[UNR], ec2[UNR];
  unsigned bits[UNR];
};

template <int BM, int BN, int NT, int EPI>
__device__ __forceinline__ void epi_load_batch(const IgemmArgs& p, int m0, int n0, int it0,
                                               EpiBatch<epi_unr<BM, BN, NT>()>& b) {
  constexpr int UNR = epi_unr<BM, BN, NT>();
  constexpr int CPR = BN / 8, RSTEP = NT / CPR;
  constexpr bool two = EPI == 5;
  constexpr bool EA = EPI == 1 || EPI == 2 || EPI == 4 || EPI == 5;
  constexpr bool EB = EPI == 2 || EPI == 3;
  constexpr bool EC = EPI == 4 || EPI == 5;
  const int tid = threadIdx.x;
  const int ch = tid % CPR, r0 = tid / CPR;
  const int n = n0 + ch * 8;
  const int OHW = p.OH * p.OW;
#pragma unroll
  for (int u = 0; u < UNR; ++u) {
    const int row = r0 + (it0 + u) * RSTEP;
    const int m = m0 + row;
    b.ok[u] = m < p.M && n < p.N;
    size_t oo;
    if (p.direct_out) {
      oo = (size_t)m * p.ldo + n;
    } else {
      const int img = m / OHW;
      const int rem = m - img * OHW;
      const int oh = rem / p.OW;
      const int ow = rem - oh * p.OW;
      oo = ((size_t)(img * p.OHp + oh * p.osh + p.ooh) * p.OWp + (ow * p.osw + p.oow)) * p.ldo + n;
    }
    b.o[u] = b.ok[u] ? oo : 0;  // a dead lane reads element 0 and stores nothing
    // streamed operands: read once, nontemporal (no L2 allocation for 0.1-0.5 GB tensors)
    if (EA) {
      if (p.epi_a_sub) {
        // the residual lives only at even (oh, ow): a stride-2 1x1 downsample's dgrad, kept
        // compact instead of zero-filling the full-resolution tensor (host: direct output)
        const int img = m / OHW;
        const int rem = m - img * OHW;
        const int oh = rem / p.OW;
        const int ow = rem - oh * p.OW;
        const bool on = b.ok[u] && !((oh | ow) & 1);
        const size_t oc = ((size_t)(img * ((p.OH + 1) >> 1) + (oh >> 1)) * ((p.OW + 1) >> 1) +
                           (ow >> 1)) * p.ldo + n;
        b.ea[u] = on ? __builtin_nontemporal_load((const u32x4*)(p.epi_a + oc))
                     : (u32x4){0u, 0u, 0u, 0u};
      } else {
        b.ea[u] = __builtin_nontemporal_load((const u32x4*)(p.epi_a + b.o[u]));
      }
    }
    if (EC) b.ec[u] = __builtin_nontemporal_load((const u32x4*)(p.epi_c + b.o[u]));
    if (two) b.ec2[u] = *(const u32x4*)(p.epi_c2 + b.o[u]);
    if (EB) {
      b.eb[u] = *(const u32x4*)(p.epi_b + b.o[u]);
    } else if (EC) {
      if (p.epi_mask != nullptr) {
        b.bits[u] = p.epi_mask[b.o[u] >> 3];
      } else {
        const u32x4 y = *(const u32x4*)(p.epi_b + b.o[u]);
        unsigned bb = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e)
          bb |= (lo_bf(y[e]) > 0.f ? 1u : 0u) << (2 * e) | (hi_bf(y[e]) > 0.f ? 2u : 0u) << (2 * e);
        b.bits[u] = bb;
      }
    }
  }
}

// Epilogue prefetch: the residual-gradient modes (4/5: three streamed operands per output row,
// the HBM-heaviest epilogue) load their first row batch before the main loop, so its latency
// overlaps the operand DMA of the (short-K) GEMM instead of following it.
template <int EPI>
constexpr bool epi_prefetch() { return EPI == 3 || EPI == 4 || EPI == 5; }

template <int BM, int BN, int WM, int WN, int NT, int EPI>
__device__ __forceinline__ void igemm_epilogue(const IgemmArgs& p,
                                               f32x4 (&acc)[BM / WM / 16][BN / WN / 16],
                                               char* smem, int m0, int n0, int mb,
                                               const EpiBatch<epi_unr<BM, BN, NT>()>* pre = nullptr) {
  constexpr int TM = BM / WM, TN = BN / WN;
  constexpr int FM = TM / 16, FN = TN / 16;
  static_assert(BN / 8 <= NT && NT % (BN / 8) == 0 && BN <= NT, "epilogue thread mapping");
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int wm = wid / WN, wn = wid % WN;
  const int OHW = p.OH * p.OW;
  constexpr int CST = BN + 8;  // padded row stride (elements)
  uint16_t* Cs = (uint16_t*)smem;
  // the MFMAs compute C^T fragments (B operand first), so each lane holds 4 consecutive
  // channels of one output row: one 8-byte LDS store per fragment instead of four 2-byte ones
#pragma unroll
  for (int fn = 0; fn < FN; ++fn) {
    const int col = wn * TN + fn * 16 + (lane >> 4) * 4;
    float bv[4] = {0.f, 0.f, 0.f, 0.f};
    if (p.bias != nullptr && n0 + col < p.N) {
#pragma unroll
      for (int i = 0; i < 4; ++i) bv[i] = p.bias[n0 + col + i];
    }
#pragma unroll
    for (int fm = 0; fm < FM; ++fm) {
      const int row = wm * TM + fm * 16 + (lane & 15);
      const u32x2 w = {pack2bf(acc[fm][fn][0] + bv[0], acc[fm][fn][1] + bv[1]),
                       pack2bf(acc[fm][fn][2] + bv[2], acc[fm][fn][3] + bv[3])};
      *(u32x2*)(Cs + row * CST + col) = w;
    }
  }
  __syncthreads();
  constexpr int CPR = BN / 8;            // 16-B chunks per row
  constexpr int RSTEP = NT / CPR;        // rows per pass
  const int ch = tid % CPR;
  const int r0 = tid / CPR;
  float s1[8], s2[8], s3[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) { s1[e] = 0.f; s2[e] = 0.f; s3[e] = 0.f; }
  constexpr bool two = EPI == 5;  // mode 4 + the producer's downsample-BN stream
  const int n = n0 + ch * 8;
  const int seg = p.seg_rows > 0 ? m0 / p.seg_rows : 0;  // block-uniform (host guarantees)
  float esc[8], esh[8], emu[8], einv[8], emu2[8], einv2[8];
  if (EPI == 3 || EPI == 4 || EPI == 5) {
    const int S = p.epi_S;
    const int cb = n < p.N ? n : 0;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      if (EPI == 3) {
        esc[e] = p.epi_ss[seg * p.N + cb + e];
        esh[e] = p.epi_ss[(S + seg) * p.N + cb + e];
      }
      emu[e] = p.epi_mi[seg * p.N + cb + e];
      einv[e] = p.epi_mi[(S + seg) * p.N + cb + e];
      if (two) {
        emu2[e] = p.epi_mi2[seg * p.N + cb + e];
        einv2[e] = p.epi_mi2[(S + seg) * p.N + cb + e];
      }
    }
  }
  // rows in batches of UNR with every global operand load of the batch issued before any is
  // consumed: one row at a time left ~1 load set in flight per wave and ran at ~3.5 TB/s
  constexpr int NIT = BM / RSTEP;
  constexpr int UNR = epi_unr<BM, BN, NT>();
  static_assert(NIT % UNR == 0, "epilogue batches");
  // software-pipelined: the next batch's operand loads are issued before this batch is
  // processed and stored, so a block keeps two batches of streamed operands in flight (the
  // residual-gradient modes read ~2x what they write; one batch at a time exposed a full
  // memory latency per batch).  The accumulators are dead here (staged in Cs), so the second
  // batch's registers are free.
  EpiBatch<UNR> Bn;
  if (pre != nullptr)
    Bn = *pre;
  else
    epi_load_batch<BM, BN, NT, EPI>(p, m0, n0, 0, Bn);
  for (int it0 = 0; it0 < NIT; it0 += UNR) {
    const EpiBatch<UNR> B = Bn;
    if (it0 + UNR < NIT) epi_load_batch<BM, BN, NT, EPI>(p, m0, n0, it0 + UNR, Bn);
    const size_t* o = B.o;
    const bool* ok = B.ok;
    const u32x4* ea = B.ea;
    const u32x4* eb = B.eb;
    const u32x4* ec = B.ec;
    const u32x4* ec2 = B.ec2;
    const unsigned* bits = B.bits;
    u32x4 v[UNR];
#pragma unroll
    for (int u = 0; u < UNR; ++u) v[u] = *(const u32x4*)(Cs + (r0 + (it0 + u) * RSTEP) * CST + ch * 8);
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      if (!ok[u]) continue;
      u32x4 w = v[u];
      if (EPI == 1) {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          w[e] = pack2bf(lo_bf(w[e]) + lo_bf(ea[u][e]), hi_bf(w[e]) + hi_bf(ea[u][e]));
      } else if (EPI == 2) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float a = lo_bf(eb[u][e]) > 0.f ? lo_bf(ea[u][e]) : 0.f;
          const float b = hi_bf(eb[u][e]) > 0.f ? hi_bf(ea[u][e]) : 0.f;
          w[e] = pack2bf(lo_bf(w[e]) + a, hi_bf(w[e]) + b);
        }
      } else if (EPI == 3) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float y0 = lo_bf(eb[u][e]), y1 = hi_bf(eb[u][e]);
          const float g0 = y0 * esc[2 * e] + esh[2 * e] > 0.f ? lo_bf(w[e]) : 0.f;
          const float g1 = y1 * esc[2 * e + 1] + esh[2 * e + 1] > 0.f ? hi_bf(w[e]) : 0.f;
          w[e] = pack2bf(g0, g1);  // exact: g is 0 or an already-rounded bf16 value
          if (p.stats != nullptr) {
            s1[2 * e] += g0; s2[2 * e] += g0 * ((y0 - emu[2 * e]) * einv[2 * e]);
            s1[2 * e + 1] += g1; s2[2 * e + 1] += g1 * ((y1 - emu[2 * e + 1]) * einv[2 * e + 1]);
          }
        }
      } else if (EPI == 4 || EPI == 5) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const uint32_t sum =
              pack2bf(lo_bf(w[e]) + lo_bf(ea[u][e]), hi_bf(w[e]) + hi_bf(ea[u][e]));
          const float g0 = (bits[u] >> (2 * e)) & 1u ? lo_bf(sum) : 0.f;
          const float g1 = (bits[u] >> (2 * e + 1)) & 1u ? hi_bf(sum) : 0.f;
          w[e] = pack2bf(g0, g1);
          if (p.stats != nullptr) {
            s1[2 * e] += g0; s2[2 * e] += g0 * ((lo_bf(ec[u][e]) - emu[2 * e]) * einv[2 * e]);
            s1[2 * e + 1] += g1;
            s2[2 * e + 1] += g1 * ((hi_bf(ec[u][e]) - emu[2 * e + 1]) * einv[2 * e + 1]);
          }
          if (two) {
            s3[2 * e] += g0 * ((lo_bf(ec2[u][e]) - emu2[2 * e]) * einv2[2 * e]);
            s3[2 * e + 1] += g1 * ((hi_bf(ec2[u][e]) - emu2[2 * e + 1]) * einv2[2 * e + 1]);
          }
        }
      }
      __builtin_nontemporal_store(w, (u32x4*)(p.out + o[u]));
      if (EPI < 3 && p.stats != nullptr) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float a = lo_bf(w[e]), b = hi_bf(w[e]);
          s1[2 * e] += a; s2[2 * e] += a * a;
          s1[2 * e + 1] += b; s2[2 * e + 1] += b * b;
        }
      }
    }
  }
  if (p.stats != nullptr) {
    // lanes of a wave that share a column chunk (tid % CPR) sum their rows with cross-lane
    // xor-shuffles first; only one partial per wave goes through LDS
    constexpr int NS = two ? 3 : 2;
    constexpr int NWV = NT / 64;
#pragma unroll
    for (int off = CPR; off < 64; off <<= 1) {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        s1[e] += __shfl_xor(s1[e], off, 64);
        s2[e] += __shfl_xor(s2[e], off, 64);
        if (two) s3[e] += __shfl_xor(s3[e], off, 64);
      }
    }
    __syncthreads();
    float* red = (float*)smem;  // [NWV][BN][NS]
    if (lane < CPR) {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        red[(wid * BN + ch * 8 + e) * NS + 0] = s1[e];
        red[(wid * BN + ch * 8 + e) * NS + 1] = s2[e];
        if (two) red[(wid * BN + ch * 8 + e) * NS + 2] = s3[e];
      }
    }
    __syncthreads();
    if (tid < BN && n0 + tid < p.N) {
      float a = 0.f, b = 0.f, d = 0.f;
#pragma unroll
      for (int r = 0; r < NWV; ++r) {
        a += red[(r * BN + tid) * NS + 0];
        b += red[(r * BN + tid) * NS + 1];
        if (two) d += red[(r * BN + tid) * NS + 2];
      }
      const int blk = p.stats_seg_blocks > 0
                          ? seg * p.stats_seg_blocks + p.stats_base + (m0 - seg * p.seg_rows) / BM
                          : mb;
      p.stats[((size_t)blk * 2 + 0) * p.N + n0 + tid] = a;
      p.stats[((size_t)blk * 2 + 1) * p.N + n0 + tid] = b;
      if (two) {
        p.stats2[((size_t)blk * 2 + 0) * p.N + n0 + tid] = a;
        p.stats2[((size_t)blk * 2 + 1) * p.N + n0 + tid] = d;
      }
    }
  }
}

// PRO: 0 none, 1 BN-apply + ReLU prologue, 2 BN-backward prologue (two operands)
template <int BM, int BN, int WM, int WN, int PRO, int EPI>
__global__ __launch_bounds__(256, (BM * BN > 128 * 128) ? 1 : 2) void igemm_nt(IgemmArgs p) {
  constexpr int TM = BM / WM, TN = BN / WN;
  constexpr int FM = TM / 16, FN = TN / 16;
  constexpr int ACH = BM * 8 / 256;
  constexpr int BCH = BN * 8 / 256;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  uint16_t* As = (uint16_t*)smem;          // [2][BM][64]
  // one staging buffer when the whole K fits one tile (the HBM-bound 1x1 convs): the smaller
  // LDS footprint admits more resident blocks to overlap their load and store phases
  uint16_t* Bs = As + (p.K > 64 ? 2 : 1) * BM * 64;  // [stages][BN][64]

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int wm = wid / WN, wn = wid % WN;
  const int lbid = xcd_remap(blockIdx.x, gridDim.x);
  const int mb = lbid / p.nNb, nb = lbid % p.nNb;
  const int m0 = mb * BM, n0 = nb * BN;

  const __amdgpu_buffer_rsrc_t ra_src = buf_rsrc(p.A, p.a_bytes);
  const __amdgpu_buffer_rsrc_t rb_src = buf_rsrc(p.B, p.b_bytes);

  const int cch = tid & 7;
  const int rbase = tid >> 3;
  const int OHW = p.OH * p.OW;
  int a_n[ACH], a_ih[ACH], a_iw[ACH];
  bool a_ok[ACH];
#pragma unroll
  for (int j = 0; j < ACH; ++j) {
    const int m = m0 + rbase + 32 * j;
    a_ok[j] = m < p.M;
    const int mm = a_ok[j] ? m : 0;
    const int n = mm / OHW;
    const int rem = mm - n * OHW;
    const int oh = rem / p.OW;
    const int ow = rem - oh * p.OW;
    a_n[j] = n;
    a_ih[j] = oh * p.ish + p.ih0;
    a_iw[j] = ow * p.isw + p.iw0;
  }
  int b_off[BCH];
  bool b_ok[BCH];
#pragma unroll
  for (int j = 0; j < BCH; ++j) {
    const int nrow = n0 + rbase + 32 * j;
    b_ok[j] = nrow < p.N;
    b_off[j] = nrow * p.K;
  }

  u32x4 ra[ACH], rb[BCH], ra2[ACH];
  bool rok[ACH];
  float psc[8], psh[8], pdd[8];
  constexpr bool pro = PRO == 1;
  constexpr bool bnb = PRO == 2;
  const int pseg = (pro || bnb) ? m0 / p.pro_seg_rows : 0;  // block-uniform (host guarantees)
  const __amdgpu_buffer_rsrc_t ra2_src = buf_rsrc(bnb ? p.A2 : p.A, p.a_bytes);
  const uint32_t OOB_A = p.a_bytes, OOB_B = p.b_bytes;

  auto gload = [&](int kt) {
    const int k = kt * 64 + cch * 8;
    const bool kok = k < p.K;
    const int tap = k / p.C;
    const int ci = k - tap * p.C;
    const int kh = tap / p.KW;
    const int kw = tap - kh * p.KW;
#pragma unroll
    for (int j = 0; j < ACH; ++j) {
      const int ih = a_ih[j] + kh * p.dh;
      const int iw = a_iw[j] + kw * p.dw;
      const bool ok = a_ok[j] && kok && (unsigned)ih < (unsigned)p.IH && (unsigned)iw < (unsigned)p.IW;
      rok[j] = ok;
      const uint32_t off = ok ? (uint32_t)((((a_n[j] * p.IH + ih) * p.IW + iw) * p.C + ci) * 2) : OOB_A;
      ra[j] = __builtin_amdgcn_raw_buffer_load_b128(ra_src, off, 0, 0);
      if (bnb) ra2[j] = __builtin_amdgcn_raw_buffer_load_b128(ra2_src, off, 0, 0);
    }
    if (pro || bnb) {
      const int cc = kok ? ci : 0;
      const float4* ps = (const float4*)(p.pro_sc + pseg * p.C + cc);
      const float4* ph = (const float4*)(p.pro_sh + pseg * p.C + cc);
      const float4 s0 = ps[0], s1 = ps[1], h0 = ph[0], h1 = ph[1];
      psc[0] = s0.x; psc[1] = s0.y; psc[2] = s0.z; psc[3] = s0.w;
      psc[4] = s1.x; psc[5] = s1.y; psc[6] = s1.z; psc[7] = s1.w;
      psh[0] = h0.x; psh[1] = h0.y; psh[2] = h0.z; psh[3] = h0.w;
      psh[4] = h1.x; psh[5] = h1.y; psh[6] = h1.z; psh[7] = h1.w;
      if (bnb) {
        const float4* pq = (const float4*)(p.pro_d + pseg * p.C + cc);
        const float4 d0 = pq[0], d1 = pq[1];
        pdd[0] = d0.x; pdd[1] = d0.y; pdd[2] = d0.z; pdd[3] = d0.w;
        pdd[4] = d1.x; pdd[5] = d1.y; pdd[6] = d1.z; pdd[7] = d1.w;
      }
    }
#pragma unroll
    for (int j = 0; j < BCH; ++j) {
      const uint32_t off = (b_ok[j] && kok) ? (uint32_t)((b_off[j] + k) * 2) : OOB_B;
      rb[j] = __builtin_amdgcn_raw_buffer_load_b128(rb_src, off, 0, 0);
    }
  };
  auto lstore = [&](int buf) {
#pragma unroll
    for (int j = 0; j < ACH; ++j) {
      const int row = rbase + 32 * j;
      const int ch = cch ^ (row & 7);
      const u32x4 v = pro   ? affine_relu8(ra[j], psc, psh, rok[j], p.pro_relu != 0)
                      : bnb ? bnbwd8(ra[j], ra2[j], psc, psh, pdd, rok[j])
                            : ra[j];
      *(u32x4*)(As + buf * BM * 64 + row * 64 + ch * 8) = v;
    }
#pragma unroll
    for (int j = 0; j < BCH; ++j) {
      const int row = rbase + 32 * j;
      const int ch = cch ^ (row & 7);
      *(u32x4*)(Bs + buf * BN * 64 + row * 64 + ch * 8) = rb[j];
    }
  };

  f32x4 acc[FM][FN];
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

  const int nk = (p.K + 63) / 64;
  gload(0);
  lstore(0);
  __syncthreads();
  for (int kt = 0; kt < nk; ++kt) {
    const int cur = kt & 1;
    if (kt + 1 < nk) gload(kt + 1);
    const uint16_t* Ab = As + cur * BM * 64;
    const uint16_t* Bb = Bs + cur * BN * 64;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      bf16x8 af[FM], bfr[FN];
#pragma unroll
      for (int fm = 0; fm < FM; ++fm) {
        const int row = wm * TM + fm * 16 + (lane & 15);
        const int ch = (ks * 4 + (lane >> 4)) ^ (row & 7);
        af[fm] = *(const bf16x8*)(Ab + row * 64 + ch * 8);
      }
#pragma unroll
      for (int fn = 0; fn < FN; ++fn) {
        const int row = wn * TN + fn * 16 + (lane & 15);
        const int ch = (ks * 4 + (lane >> 4)) ^ (row & 7);
        bfr[fn] = *(const bf16x8*)(Bb + row * 64 + ch * 8);
      }
#pragma unroll
      for (int fm = 0; fm < FM; ++fm)
#pragma unroll
        for (int fn = 0; fn < FN; ++fn)
          acc[fm][fn] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bfr[fn], af[fm], acc[fm][fn], 0, 0, 0);
    }
    if (kt + 1 < nk) lstore(cur ^ 1);
    __syncthreads();
  }

  igemm_epilogue<BM, BN, WM, WN, 256, EPI>(p, acc, smem, m0, n0, mb);
}

// 16-byte buffer load straight into LDS (buffer_load_dwordx4 ... lds): lane l's bytes land at
// lds + 16*l (wave-uniform base); an out-of-range offset writes zeros.  The builtin exists only
// in the device pass (the host pass of a kernel that names it would drop the kernel's stub).
__device__ __forceinline__ void dma16(__amdgpu_buffer_rsrc_t r, const void* lds, uint32_t off) {
#if defined(__HIP_DEVICE_COMPILE__)
  __builtin_amdgcn_raw_ptr_buffer_load_lds(r, LDS_PTR(void, lds), 16, off, 0, 0, 0);
#endif
}

// The same DMA, opaque to hipcc's wait-count pass.  That pass cannot tell which LDS bytes an
// in-flight buffer_load ... lds writes, so it puts s_waitcnt vmcnt(0) in front of the first
// LDS store (the in-LDS prologues) or ds_read_b64_tr_b16 (the weight gradients) that follows
// the builtin — draining the NEXT tile's DMA before the current tile computes, i.e. no
// pipelining at all (tools/isa_check.py finds those drains in the disassembly).  The kernels
// that use this form order their DMA themselves: a manual vmcnt wait + raw barrier at the top
// of every k-step covers the landed tile, and the buffer being refilled was released by that
// barrier.  Compiler-generated vmcnt waits for other loads stay correct (ops hidden from the
// counter only make its counted waits stricter).  M0 holds the wave-uniform LDS base; these
// kernels have no other M0 user (checked by tools/isa_check.py), and the s_nop covers the
// M0-write → LDS-DMA hazard.
__device__ __forceinline__ void dma16_opaque(__amdgpu_buffer_rsrc_t r, const void* lds,
                                             uint32_t off) {
#if defined(__HIP_DEVICE_COMPILE__)
  const uint32_t base = __builtin_amdgcn_readfirstlane(
      (uint32_t)(uintptr_t)LDS_PTR(const void, lds));
  asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tbuffer_load_dwordx4 %0, %1, 0 offen lds"
               :: "v"(off), "s"(r), "s"(base) : "memory");
#endif
}

// ---------------------------------------------------------------------- igemm, LDS-DMA staged
// Large-tile implicit GEMM for the compute-bound convolutions (no operand prologue): both
// operands go HBM/L2 → LDS with buffer_load_dwordx4 … lds (no VGPR round trip, no ds_write
// pass; the LDS-write pass was the register-staged kernel's co-bottleneck with the ds_reads).
// One wave-instruction fills 8 rows x 128 B of the [rows][64] tile image; the XOR chunk swizzle
// of the image is produced by permuting each lane's SOURCE chunk (the LDS side of a DMA is
// lane-linear), so fragment reads are the same conflict-free ds_read_b128 as igemm_nt.
// Out-of-range rows / padding taps use an out-of-range buffer offset: the DMA writes zeros.
// Pipeline: 2 LDS stages, BK = 64; the DMA of tile k+1 is issued right after the barrier that
// publishes tile k and runs under tile k's MFMAs; one vmcnt(0) + barrier per k-tile.
// Host guarantees: C % 64 == 0 (a 64-wide K slice is one tap), no prologue.
// byte offset of igemm_glds's prologue table: after the larger of the staging buffers, the
// epilogue's C image and its statistics scratch (na = 2: the block-output prologue stages the
// residual tile next to the A tile)
__host__ __device__ constexpr size_t igemm_glds_pro_offset(int BM, int BN, int NT, int st,
                                                           int na = 1) {
  return ((size_t)st * (na * BM + BN) * 64 * 2 > (size_t)BM * (BN + 8) * 2
              ? ((size_t)st * (na * BM + BN) * 64 * 2 > (size_t)(NT / (BN / 8)) * BN * 3 * 4
                     ? (size_t)st * (na * BM + BN) * 64 * 2
                     : (size_t)(NT / (BN / 8)) * BN * 3 * 4)
              : ((size_t)BM * (BN + 8) * 2 > (size_t)(NT / (BN / 8)) * BN * 3 * 4
                     ? (size_t)BM * (BN + 8) * 2
                     : (size_t)(NT / (BN / 8)) * BN * 3 * 4));
}

// PRO == 1 (1x1 convolutions without padding only, host-checked): the previous BatchNorm's
// normalise + ReLU is applied to the A tile in LDS after the DMA lands (one read-modify-write
// pass and one extra barrier per k-tile), so the conv3 forward keeps the DMA pipeline too.
// PRO == 3 (1x1 / stride 1 / unpadded, 2 stages, host-checked): the A operand is the previous
// block's output, never materialised by a separate pass — the DMA lands both of its inputs
// (pre-BN conv3 activation and residual) and the prologue pass forms the block output in LDS
// for the MFMAs and streams it (plus its ReLU bitmask) to HBM from the nb == 0 blocks.  The
// separate BN-apply kernel and the GEMM's re-read of its output are gone (reference
// models/resnet.py Bottleneck.forward: out = relu(bn3(conv3) + shortcut), then conv1 of the
// next block).
// NST == 3: three LDS stages; the DMA of tile k+2 is issued while tile k computes and a
// counted vmcnt keeps tile k+1's DMA in flight across the (raw) barrier.
template <int BM, int BN, int WM, int WN, int PRO, int EPI, int NST>
__global__ __launch_bounds__(64 * WM * WN, NST == 1 ? 2 : 1) void igemm_glds(IgemmArgs p) {
  constexpr int NW = WM * WN, NT = 64 * NW;
  constexpr int TM = BM / WM, TN = BN / WN;
  constexpr int FM = TM / 16, FN = TN / 16;
  constexpr int AI = BM / (8 * NW), BI = BN / (8 * NW);  // DMA instructions per wave per tile
  static_assert(AI >= 1 && BI >= 1 && AI * 8 * NW == BM && BI * 8 * NW == BN, "glds tiling");
  // WN == 1 tiles: every wave owns its A rows, so PRO 1 transforms the A fragments in registers
  // after the ds_read (each element exactly once) instead of a read-modify-write pass over the
  // landed tile plus a barrier per k-tile
  constexpr bool RPRO = PRO == 1 && WN == 1;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int stages = p.K > 64 ? NST : 1;
  constexpr int NA = PRO >= 2 ? 2 : 1;  // PRO 2 / 3 stage a second A-shaped operand (Rs)
  uint16_t* As = (uint16_t*)smem;          // [stages][BM][64]
  uint16_t* Bs = As + stages * BM * 64;    // [stages][BN][64] (one stage when K <= 64)
  uint16_t* Rs = Bs + stages * BN * 64;    // PRO 3: residual / PRO 2: A2 tile, [stages][BM][64]
  // PRO: [sc, sh (, rsc, rsh)][C] of the block's segment, behind the staging buffers and the
  // epilogue image
  float* Pt = (float*)(smem + igemm_glds_pro_offset(BM, BN, 64 * WM * WN, stages, NA));

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int wm = wid / WN, wn = wid % WN;
  const int lbid = xcd_remap(blockIdx.x, gridDim.x);
  const int mb = lbid / p.nNb, nb = lbid % p.nNb;
  const int m0 = mb * BM, n0 = nb * BN;

  const __amdgpu_buffer_rsrc_t ra = buf_rsrc(p.A, p.a_bytes);
  const __amdgpu_buffer_rsrc_t rb = buf_rsrc(p.B, p.b_bytes);
  const __amdgpu_buffer_rsrc_t rr = buf_rsrc(PRO >= 2 ? p.A2 : p.A, p.a_bytes);

  // lane → (row within its 8-row piece, physical chunk); the logical chunk it fetches is
  // pch ^ (row & 7) = pch ^ lrow (every piece starts at a multiple of 8 rows)
  const int lrow = lane >> 3, pch = lane & 7;
  const int lch = pch ^ lrow;
  const int OHW = p.OH * p.OW;
  // Issue cost: every DMA address below is one add on per-thread values fixed for the whole
  // block, plus wave-uniform (scalar) per-k-tile terms.  The tap / channel walk of the k-tiles is
  // carried incrementally in scalar registers (a runtime integer division lowers to a VALU
  // reciprocal sequence even for uniform operands), the row's tap-(0, 0) offset is computed
  // once, and the LDS destinations come from the scalar wave index — the first cut spent ~40
  // VALU instructions (two quarter-rate multiplies) per DMA, comparable to the k-tile's MFMA time.
  const int wid_u = __builtin_amdgcn_readfirstlane(wid);
  int a_base[AI], a_ih[AI], a_iw[AI];
#pragma unroll
  for (int j = 0; j < AI; ++j) {
    const int m = m0 + (j * NW + wid) * 8 + lrow;
    const bool ok = m < p.M;
    const int mm = ok ? m : 0;
    const int n = mm / OHW;
    const int rem = mm - n * OHW;
    const int oh = rem / p.OW;
    const int ow = rem - oh * p.OW;
    const int ih = oh * p.ish + p.ih0, iw = ow * p.isw + p.iw0;
    // tap-(0, 0) byte offset of the lane's chunk: may lie outside the tensor for padded taps,
    // used only when the bounds test passes (int32: a_bytes < 2^31 host-checked)
    a_base[j] = ((n * p.IH + ih) * p.IW + iw) * p.C * 2 + lch * 16;
    a_ih[j] = ok ? ih : -(1 << 28);  // invalid rows fail the bounds test
    a_iw[j] = iw;
  }
  uint32_t b_off[BI];
#pragma unroll
  for (int j = 0; j < BI; ++j) {
    const int nrow = n0 + (j * NW + wid) * 8 + lrow;
    b_off[j] = nrow < p.N ? (uint32_t)(nrow * p.K + lch * 8) * 2u : p.b_bytes;
  }
  const uint32_t OOB_A = p.a_bytes;
  int nx_c = 0, nx_kh = 0, nx_kw = 0;  // channel offset and tap of the next k-tile to issue

  auto issue = [&](int kt, int buf) {  // called for kt = 0, 1, 2, ... in order
    const int dih = nx_kh * p.dh, diw = nx_kw * p.dw;
    const int delta = ((dih * p.IW + diw) * p.C + nx_c) * 2;
    nx_c += 64;
    if (nx_c == p.C) {
      nx_c = 0;
      if (++nx_kw == p.KW) { nx_kw = 0; ++nx_kh; }
    }
    uint16_t* Aw = As + buf * BM * 64 + wid_u * 8 * 64;
#pragma unroll
    for (int j = 0; j < AI; ++j) {
      const int ih = a_ih[j] + dih;
      const int iw = a_iw[j] + diw;
      const bool ok = (unsigned)ih < (unsigned)p.IH && (unsigned)iw < (unsigned)p.IW;
      const uint32_t off = ok ? (uint32_t)(a_base[j] + delta) : OOB_A;
      // the prologues store into the landed tile: the builtin DMA would be drained right
      // after its issue (see dma16_opaque), so those kernels issue it opaquely
      if (PRO) {
        dma16_opaque(ra, Aw + j * NW * 8 * 64, off);
        if (PRO >= 2)
          dma16_opaque(rr, Rs + buf * BM * 64 + wid_u * 8 * 64 + j * NW * 8 * 64, off);
      } else {
        dma16(ra, Aw + j * NW * 8 * 64, off);
      }
    }
    uint16_t* Bw = Bs + buf * BN * 64 + wid_u * 8 * 64;
    const uint32_t kb = (uint32_t)kt * 128u;
#pragma unroll
    for (int j = 0; j < BI; ++j) {
      if (PRO)
        dma16_opaque(rb, Bw + j * NW * 8 * 64, b_off[j] + kb);
      else
        dma16(rb, Bw + j * NW * 8 * 64, b_off[j] + kb);
    }
  };

  f32x4 acc[FM][FN];
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

  EpiBatch<epi_unr<BM, BN, NT>()> pre;
  if (epi_prefetch<EPI>()) epi_load_batch<BM, BN, NT, EPI>(p, m0, n0, 0, pre);
  const int nk = p.K / 64;
  if (PRO) {
    // table staged before any DMA: ordinary global loads consumed in the loop would make hipcc
    // drain the in-flight DMA (vmcnt(0)) right after it is issued
    const int pseg = m0 / p.pro_seg_rows;  // block-uniform (host guarantees)
    for (int i = tid; i < 2 * p.C; i += NT)
      Pt[i] = (i < p.C ? p.pro_sc : p.pro_sh)[pseg * p.C + (i < p.C ? i : i - p.C)];
    if (PRO == 2)  // BN-backward: a = sc·A + sh·A2 + d, the d column after sc, sh
      for (int i = tid; i < p.C; i += NT) Pt[2 * p.C + i] = p.pro_d[pseg * p.C + i];
    if (PRO == 3)  // residual scale / shift; identity residual = (1, 0)
      for (int i = tid; i < 2 * p.C; i += NT) {
        const int c = i < p.C ? i : i - p.C;
        Pt[2 * p.C + i] = p.pro_rsc != nullptr
                              ? (i < p.C ? p.pro_rsc : p.pro_rsh)[pseg * p.C + c]
                              : (i < p.C ? 1.f : 0.f);
      }
    __syncthreads();
  }
  constexpr int PER = NA * AI + BI;  // DMA instructions per wave per k-tile
  issue(0, 0);
  if (NST == 3 && nk > 1) issue(1, 1);
  for (int kt = 0; kt < nk; ++kt) {
    const int cur = NST == 3 ? kt % 3 : NST == 2 ? (kt & 1) : 0;
    if (NST == 3 && kt + 1 < nk)
      asm volatile("s_waitcnt vmcnt(%0)" ::"n"(PER) : "memory");  // tile kt+1 stays in flight
    else if (PRO == 3 && nb == 0 && kt > 0)
      // tile kt's DMA was issued before tile kt-1's block-output stores (2 per chunk, every
      // wave, M % BM == 0 host-checked): those stay in flight
      asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * BM * 8 / NT) : "memory");
    else
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    // raw barrier (__syncthreads() would drain the in-flight DMA): tile kt visible to every
    // wave, every wave done reading the buffer the next issue overwrites
    __builtin_amdgcn_s_barrier();
    if (NST > 1 && kt + NST - 1 < nk) issue(kt + NST - 1, (kt + NST - 1) % NST);
    // prologue passes over the landed tile: chunk c = tid + i·NT sits in row c / 8 and holds
    // logical channel chunk (c % 8) ^ (row % 8), the same for every i (NT % 64 == 0), so the
    // per-channel tables are read from LDS once per k-tile rather than once per chunk (LDS
    // stores into the tile keep hipcc from hoisting them itself), and every chunk of the thread
    // is loaded before the first is written back
    constexpr int PCH = BM * 8 / NT;  // chunks per thread
    static_assert(NT % 64 == 0, "prologue chunk mapping");
    const int plc = (tid & 7) ^ ((tid >> 3) & 7);
    if (PRO == 3) {
      const int ci = kt * 64 + plc * 8;  // 1x1: K = C
      float tb[4][8];  // sc, sh, rsc, rsh of the thread's 8 channels
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const float4* pt = (const float4*)(Pt + t * p.C + ci);
        const float4 t0 = pt[0], t1 = pt[1];
        tb[t][0] = t0.x; tb[t][1] = t0.y; tb[t][2] = t0.z; tb[t][3] = t0.w;
        tb[t][4] = t1.x; tb[t][5] = t1.y; tb[t][6] = t1.z; tb[t][7] = t1.w;
      }
      // (one chunk at a time here: the 8-wave 256 x 256 tile has no registers to spare)
#pragma unroll
      for (int i = 0; i < PCH; ++i) {
        const int c = tid + i * NT;
        const int row = c >> 3;
        const u32x4 v = *(const u32x4*)(As + cur * BM * 64 + c * 8);
        const u32x4 r = *(const u32x4*)(Rs + cur * BM * 64 + c * 8);
        float o[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float xv = (e & 1) ? hi_bf(v[e >> 1]) : lo_bf(v[e >> 1]);
          const float rv = (e & 1) ? hi_bf(r[e >> 1]) : lo_bf(r[e >> 1]);
          o[e] = xv * tb[0][e] + tb[1][e];
          o[e] += rv * tb[2][e] + tb[3][e];
          o[e] = fmaxf(o[e], 0.f);
        }
        u32x4 w;
#pragma unroll
        for (int e = 0; e < 4; ++e) w[e] = pack2bf(o[2 * e], o[2 * e + 1]);
        *(u32x4*)(As + cur * BM * 64 + c * 8) = w;
        if (nb == 0) {  // block-uniform: every wave issues the same 2 stores per chunk
          const size_t o8 = (size_t)(m0 + row) * p.C + ci;
          __builtin_nontemporal_store(w, (u32x4*)(p.pro_out + o8));
          unsigned bits = 0;
#pragma unroll
          for (int e = 0; e < 8; ++e) bits |= (o[e] > 0.f ? 1u : 0u) << e;
          p.pro_mask[o8 / 8] = (uint8_t)bits;
        }
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
    } else if (PRO == 2) {
      // BatchNorm backward of the layer this conv's dgrad consumes, on the landed tiles: the
      // DMA brought dY (As) and the pre-BN activation (Rs); the GEMM operand is
      // A·dY + B·x + D (1x1 unpadded only: no padding taps, K = C)
      const int ci = kt * 64 + plc * 8;
      float tb[3][8];
#pragma unroll
      for (int t = 0; t < 3; ++t) {
        const float4* pt = (const float4*)(Pt + t * p.C + ci);
        const float4 t0 = pt[0], t1 = pt[1];
        tb[t][0] = t0.x; tb[t][1] = t0.y; tb[t][2] = t0.z; tb[t][3] = t0.w;
        tb[t][4] = t1.x; tb[t][5] = t1.y; tb[t][6] = t1.z; tb[t][7] = t1.w;
      }
      u32x4 va[PCH], vr[PCH];
#pragma unroll
      for (int i = 0; i < PCH; ++i) {
        const int c = tid + i * NT;
        va[i] = *(const u32x4*)(As + cur * BM * 64 + c * 8);
        vr[i] = *(const u32x4*)(Rs + cur * BM * 64 + c * 8);
      }
#pragma unroll
      for (int i = 0; i < PCH; ++i)
        *(u32x4*)(As + cur * BM * 64 + (tid + i * NT) * 8) =
            bnbwd8(va[i], vr[i], tb[0], tb[1], tb[2], true);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
    } else if (PRO && !RPRO) {
      const int ci = kt * 64 + plc * 8;  // 1x1 (host-checked): K = C
      const float4* ps = (const float4*)(Pt + ci);
      const float4* ph = (const float4*)(Pt + p.C + ci);
      const float4 s0 = ps[0], s1 = ps[1], h0 = ph[0], h1 = ph[1];
      const f32x2 sc[4] = {{s0.x, s0.y}, {s0.z, s0.w}, {s1.x, s1.y}, {s1.z, s1.w}};
      const f32x2 sh[4] = {{h0.x, h0.y}, {h0.z, h0.w}, {h1.x, h1.y}, {h1.z, h1.w}};
      u32x4 va[PCH];
#pragma unroll
      for (int i = 0; i < PCH; ++i) va[i] = *(const u32x4*)(As + cur * BM * 64 + (tid + i * NT) * 8);
#pragma unroll
      for (int i = 0; i < PCH; ++i)
        *(u32x4*)(As + cur * BM * 64 + (tid + i * NT) * 8) =
            affine_relu8_pk(va[i], sc, sh, p.pro_relu != 0);
      // raw barrier: __syncthreads() would also drain the next tile's DMA (vmcnt(0))
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
    }
    const uint16_t* Ab = As + cur * BM * 64;
    const uint16_t* Bb = Bs + cur * BN * 64;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      bf16x8 af[FM], bfr[FN];
#pragma unroll
      for (int fm = 0; fm < FM; ++fm) {
        const int row = wm * TM + fm * 16 + (lane & 15);
        const int ch = (ks * 4 + (lane >> 4)) ^ (row & 7);
        af[fm] = *(const bf16x8*)(Ab + row * 64 + ch * 8);
      }
      if constexpr (RPRO) {
        // the lane's 8 channels (logical chunk ks*4 + lane/16 of this k-tile) are the same for
        // every fragment row: one table read per k-half, the transform on the A fragments
        const int ci = kt * 64 + (ks * 4 + (lane >> 4)) * 8;  // 1x1 (host-checked): K = C
        const float4* ps = (const float4*)(Pt + ci);
        const float4* ph = (const float4*)(Pt + p.C + ci);
        const float4 s0 = ps[0], s1 = ps[1], h0 = ph[0], h1 = ph[1];
        const f32x2 sc[4] = {{s0.x, s0.y}, {s0.z, s0.w}, {s1.x, s1.y}, {s1.z, s1.w}};
        const f32x2 sh[4] = {{h0.x, h0.y}, {h0.z, h0.w}, {h1.x, h1.y}, {h1.z, h1.w}};
#pragma unroll
        for (int fm = 0; fm < FM; ++fm)
          af[fm] = __builtin_bit_cast(
              bf16x8, affine_relu8_pk(__builtin_bit_cast(u32x4, af[fm]), sc, sh, p.pro_relu != 0));
      }
#pragma unroll
      for (int fn = 0; fn < FN; ++fn) {
        const int row = wn * TN + fn * 16 + (lane & 15);
        const int ch = (ks * 4 + (lane >> 4)) ^ (row & 7);
        bfr[fn] = *(const bf16x8*)(Bb + row * 64 + ch * 8);
      }
#pragma unroll
      for (int fm = 0; fm < FM; ++fm)
#pragma unroll
        for (int fn = 0; fn < FN; ++fn)
          acc[fm][fn] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bfr[fn], af[fm], acc[fm][fn], 0, 0, 0);
    }
    if constexpr (NST == 1) {
      // single stage (the short-K tiles that run 2 blocks per CU: the other block's MFMAs
      // cover this one's loads and epilogue): every wave done with the tile, then refill it
      if (kt + 1 < nk) {
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        issue(kt + 1, 0);
      }
    }
  }
  __syncthreads();  // the epilogue reuses the staging LDS
  igemm_epilogue<BM, BN, WM, WN, NT, EPI>(p, acc, smem, m0, n0, mb,
                                          epi_prefetch<EPI>() ? &pre : nullptr);
}

// ------------------------------------------------------------ 3x3 conv, LDS-resident patch
// 3x3 / stride-1 / pad-1 convolutions (forward, and the stride-1 dgrad, which is the same conv
// with flipped weights) at 16x16 / 32x32 resolution with 64 or 128 input channels.  The
// implicit GEMM re-fetches every input pixel once per tap (9x) from L2; with N = 64..128 output
// channels there are too few MFMAs per fetched byte to hide that (the N = 64 layer1 convs ran at
// ~0.5 PFLOP/s, L2-bound).  Here a block owns 256 output pixels = 256/OW whole rows of one
// image, DMAs the (rows + 2) x (OW + 2) x C input patch (halo included, zero padding from
// out-of-range buffer offsets) into LDS ONCE, and every tap's A fragments are read from that
// patch at shifted pixel positions; only the weight tile streams per k-step (2 LDS stages).
// Patch image: [pixel][C] with 16-byte chunk c of pixel q stored at chunk c ^ (q & 7).
// Host guarantees (igemm_variant_ok): KH = KW = 3, unit strides, ih0 = iw0 = -1, OH = IH,
// OW = IW in {16, 32}, C in {64, 128}, direct output; PRO 1: BN-apply + ReLU on the landed
// patch, padding kept zero.
// PRO 2 (BatchNorm-backward operand prologue): patch chunks per thread, at most — the second
// operand is held in registers (host: ceil(patch pixels x C/8 / threads) <= this)
constexpr int kPatchBnbChunks = 11;
template <int BN, int WM, int WN, int EPI, int PRO>
__global__ __launch_bounds__(64 * WM * WN, 1) void igemm_patch(IgemmArgs p) {
  constexpr int BM = 256;
  constexpr int NW = WM * WN, NT = 64 * NW;
  constexpr int TM = BM / WM, TN = BN / WN;
  constexpr int FM = TM / 16, FN = TN / 16;
  constexpr int BI = BN / (8 * NW);  // weight DMA instructions per wave per k-step
  static_assert(BI >= 1 && BI * 8 * NW == BN, "patch tiling");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int C = p.C, OW = p.OW;
  const int TR = BM / OW;                 // output rows per block
  const int PW = OW + 2, PP = (TR + 2) * PW;  // patch width / pixels
  const int ppi = 64 / (C / 8);           // patch pixels per 1 KiB DMA instruction
  const int ninstr = (PP + ppi - 1) / ppi;
  uint16_t* Ps = (uint16_t*)smem;         // [PP][C], rounded up to whole DMA instructions
  uint16_t* Bs = Ps + ninstr * 512;       // [2][BN][64] (the last patch DMA's tail lands before)

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int wm = wid / WN, wn = wid % WN;
  const int lbid = xcd_remap(blockIdx.x, gridDim.x);
  const int mb = lbid / p.nNb, nb = lbid % p.nNb;
  const int m0 = mb * BM, n0 = nb * BN;
  const int OHW = p.OH * OW;
  const int img = m0 / OHW;
  const int row0 = (m0 - img * OHW) / OW;

  const __amdgpu_buffer_rsrc_t ra = buf_rsrc(p.A, p.a_bytes);
  const __amdgpu_buffer_rsrc_t rb = buf_rsrc(p.B, p.b_bytes);

  const int CPP = C / 8;
  // PRO: chunk c = tid + i·NT of the landed patch sits in pixel q = tid/CPP + i·(NT/CPP) at
  // physical chunk tid % CPP (NT % CPP == 0); NT/CPP is a multiple of 8, so q & 7 — and with it
  // the logical channel chunk (pch ^ (q & 7)) — is the same for every i: the thread's 8 scale /
  // shift pairs are loaded once, before the DMA (a global load consumed after it would drain
  // it), and the pixel walk is incremental (no per-chunk division by the patch width)
  f32x2 psc2[4], psh2[4];
  float pa[8], pb[8], pd[8];  // PRO 2: the BatchNorm-backward coefficients of the thread's chunk
  if (PRO == 2) {
    const int pseg = m0 / p.pro_seg_rows;
    const int ch = ((tid % CPP) ^ ((tid / CPP) & 7)) * 8;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      pa[e] = p.pro_sc[pseg * C + ch + e];
      pb[e] = p.pro_sh[pseg * C + ch + e];
      pd[e] = p.pro_d[pseg * C + ch + e];
    }
  } else if (PRO) {
    const int pseg = m0 / p.pro_seg_rows;  // block-uniform (host guarantees)
    const int ch = ((tid % CPP) ^ ((tid / CPP) & 7)) * 8;
    const float4* ps = (const float4*)(p.pro_sc + pseg * C + ch);
    const float4* ph = (const float4*)(p.pro_sh + pseg * C + ch);
    const float4 s0 = ps[0], s1 = ps[1], h0 = ph[0], h1 = ph[1];
    psc2[0] = {s0.x, s0.y}; psc2[1] = {s0.z, s0.w}; psc2[2] = {s1.x, s1.y}; psc2[3] = {s1.z, s1.w};
    psh2[0] = {h0.x, h0.y}; psh2[1] = {h0.z, h0.w}; psh2[2] = {h1.x, h1.y}; psh2[3] = {h1.z, h1.w};
  }
  // ---- patch DMA: one wave-instruction = 1 KiB = 64 lanes x 16 B (8 or 16 chunks per pixel)
  for (int i = wid; i < ninstr; i += NW) {
    const int q = i * ppi + lane / CPP;  // patch pixel
    const int pch = lane % CPP;
    const int lch = pch ^ (q & 7);
    const int pr = q / PW, pc = q - (q / PW) * PW;
    const int ih = row0 - 1 + pr, iw = pc - 1;
    const bool ok = q < PP && (unsigned)ih < (unsigned)p.IH && (unsigned)iw < (unsigned)p.IW;
    const uint32_t off =
        ok ? (uint32_t)((((img * p.IH + ih) * p.IW + iw) * C + lch * 8) * 2) : p.a_bytes;
    dma16(ra, Ps + i * 512, off);  // 512 elements = 1 KiB per instruction
  }
  // PRO 2: the second BatchNorm-backward operand (the pre-BN activation) of every chunk this
  // thread transforms, loaded to registers under the patch DMA (host: <= kPatchBnbChunks each)
  u32x4 a2v[kPatchBnbChunks];
  if (PRO == 2) {
    const __amdgpu_buffer_rsrc_t r2 = buf_rsrc(p.A2, p.a_bytes);
    const int QS = NT / CPP, q0 = tid / CPP;
    const int lch = (tid % CPP) ^ (q0 & 7);  // the same logical chunk for every i (QS % 8 == 0)
#pragma unroll
    for (int i = 0; i < kPatchBnbChunks; ++i) {
      const int q = q0 + i * QS;
      const int pr = q / PW, pc = q - (q / PW) * PW;
      const int ih = row0 - 1 + pr, iw = pc - 1;
      const bool ok = q < PP && (unsigned)ih < (unsigned)p.IH && (unsigned)iw < (unsigned)p.IW;
      const uint32_t off =
          ok ? (uint32_t)((((img * p.IH + ih) * p.IW + iw) * C + lch * 8) * 2) : p.a_bytes;
      a2v[i] = __builtin_amdgcn_raw_buffer_load_b128(r2, off, 0, 0);
    }
  }
  // ---- weight tiles
  const int lrow = lane >> 3, lbch = (lane & 7) ^ (lane >> 3);
  uint32_t b_off[BI];
#pragma unroll
  for (int j = 0; j < BI; ++j) {
    const int nrow = n0 + (j * NW + wid) * 8 + lrow;
    b_off[j] = nrow < p.N ? (uint32_t)(nrow * p.K + lbch * 8) * 2u : p.b_bytes;
  }
  auto issue_b = [&](int kt, int buf) {
#pragma unroll
    for (int j = 0; j < BI; ++j)
      dma16(rb, Bs + buf * BN * 64 + (j * NW + wid) * 8 * 64, b_off[j] + (uint32_t)(kt * 64) * 2u);
  };

  if (PRO == 2) {
    // before the accumulators and the epilogue prefetch exist (their registers and the held
    // second operand are never live together): weight tile 0 joins the patch in flight, then
    // the BatchNorm backward A·g + B·a + D of the conv's own output gradient, once per patch
    // pixel on the landed patch (padding stays zero); the block's own pixels of it are also
    // the materialised gradient the weight gradient reads (pro_out, column-0 blocks only)
    issue_b(0, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // patch + second operand + weight tile 0
    __builtin_amdgcn_s_barrier();
    const int QS = NT / CPP, q0 = tid / CPP;
    const int lch = (tid % CPP) ^ (q0 & 7);
    uint16_t* base = Ps + tid * 8;
    const bool store = p.pro_out != nullptr && nb == 0;
#pragma unroll
    for (int i = 0; i < kPatchBnbChunks; ++i) {
      const int q = q0 + i * QS;
      const int pr = q / PW, pc = q - (q / PW) * PW;
      const int ih = row0 - 1 + pr, iw = pc - 1;
      const bool ok = q < PP && (unsigned)ih < (unsigned)p.IH && (unsigned)iw < (unsigned)p.IW;
      if (ok) {
        const u32x4 w = bnbwd8(*(const u32x4*)(base + (size_t)i * NT * 8), a2v[i], pa, pb, pd,
                               true);
        *(u32x4*)(base + (size_t)i * NT * 8) = w;
        if (store && pr >= 1 && pr <= TR)
          *(u32x4*)(p.pro_out + (((size_t)img * p.IH + ih) * p.IW + iw) * C + lch * 8) = w;
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
  }
  f32x4 acc[FM][FN];
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

  // per-fragment output pixel (tile-local row r, col c) of this lane's A rows
  int frow[FM], fcol[FM];
#pragma unroll
  for (int fm = 0; fm < FM; ++fm) {
    const int m = wm * TM + fm * 16 + (lane & 15);
    frow[fm] = m / OW;
    fcol[fm] = m - frow[fm] * OW;
  }
  EpiBatch<epi_unr<BM, BN, NT>()> pre;
  if (epi_prefetch<EPI>()) epi_load_batch<BM, BN, NT, EPI>(p, m0, n0, 0, pre);
  const int nk = p.K / 64;
  if (PRO != 2) issue_b(0, 0);
  for (int kt = 0; kt < nk; ++kt) {
    const int cur = kt & 1;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // patch (first step) + weight tile kt
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    if (PRO == 1 && kt == 0) {
      // the previous BatchNorm's normalise + ReLU, once per patch pixel on the landed patch
      // (no DMA in flight here); the zero padding of out-of-image pixels stays exactly zero.
      // Four chunks per batch: their LDS reads are all issued before the first write-back.
      const int QS = NT / CPP;                    // pixel stride of the thread's chunks
      const int dr = QS / PW, dc = QS - dr * PW;  // ... as (patch rows, patch columns)
      const int q0 = tid / CPP;
      int pr = q0 / PW, pc = q0 - pr * PW;
      uint16_t* base = Ps + tid * 8;              // chunk i at base + i·NT·8
      const bool relu = p.pro_relu != 0;
      for (int i0 = 0; i0 * QS + q0 < PP; i0 += 4) {
        u32x4 v[4];
        bool ok[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int ih = row0 - 1 + pr, iw = pc - 1;
          ok[u] = (i0 + u) * QS + q0 < PP && (unsigned)ih < (unsigned)p.IH &&
                  (unsigned)iw < (unsigned)p.IW;
          if (ok[u]) v[u] = *(const u32x4*)(base + (size_t)(i0 + u) * NT * 8);
          pr += dr;
          pc += dc;
          if (pc >= PW) { pc -= PW; ++pr; }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
          if (ok[u])
            *(u32x4*)(base + (size_t)(i0 + u) * NT * 8) = affine_relu8_pk(v[u], psc2, psh2, relu);
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
    }
    if (kt + 1 < nk) issue_b(kt + 1, cur ^ 1);
    const int k0 = kt * 64;
    const int tap = k0 / C;
    const int cb = (k0 - tap * C) / 8;  // first logical chunk of this k-step in the pixel
    const int kh = tap / 3, kw = tap - (tap / 3) * 3;
    const uint16_t* Bb = Bs + cur * BN * 64;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      bf16x8 af[FM], bfr[FN];
#pragma unroll
      for (int fm = 0; fm < FM; ++fm) {
        const int q = (frow[fm] + kh) * PW + fcol[fm] + kw;
        const int ch = (cb + ks * 4 + (lane >> 4)) ^ (q & 7);
        af[fm] = *(const bf16x8*)(Ps + q * C + ch * 8);
      }
#pragma unroll
      for (int fn = 0; fn < FN; ++fn) {
        const int row = wn * TN + fn * 16 + (lane & 15);
        const int ch = (ks * 4 + (lane >> 4)) ^ (row & 7);
        bfr[fn] = *(const bf16x8*)(Bb + row * 64 + ch * 8);
      }
#pragma unroll
      for (int fm = 0; fm < FM; ++fm)
#pragma unroll
        for (int fn = 0; fn < FN; ++fn)
          acc[fm][fn] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bfr[fn], af[fm], acc[fm][fn], 0, 0, 0);
    }
  }
  __syncthreads();  // the epilogue reuses the LDS
  igemm_epilogue<BM, BN, WM, WN, NT, EPI>(p, acc, smem, m0, n0, mb,
                                          epi_prefetch<EPI>() ? &pre : nullptr);
}



// ------------------------------------------------------------------------------------ wgrad
// Physical element offset of (row r, element col) in a W-wide swizzled LDS row (see wgrad_tn):
// 4-element units are XOR-permuted by a row-dependent multiple of 4 units (so 16-byte chunks
// stay contiguous and in-row).
template <int W>
__device__ __forceinline__ int tr_swz(int r, int col) {
  const int k = W >= 128 ? ((r & 3) | (((r >> 3) & 1) << 2)) : (((r >> 1) & 1) ^ (((r >> 3) & 1) << 1));
  return ((((col >> 2) ^ (k << 2))) << 2) | (col & 3);
}

struct WgradArgs {
  const uint16_t* dY;  // [M][N] rows = forward output pixels
  const uint16_t* X;   // forward input NHWC
  float* partial;      // [splits][N][K]
  int M, N, K;
  int IH, IW, C;
  int OH, OW, KW;
  int ish, isw, dh, dw, ih0, iw0;
  uint32_t dy_bytes, x_bytes;
  int iters_per_split, splits, nCo, nKk;
  const float* pro_sc;  // X-operand prologue, [S<=2][C]
  const float* pro_sh;
  int pro_seg_rows, pro_relu, pro_S;
  // dY-operand BatchNorm-backward prologue: dY = A·dY + B·dY2 + D with coef [3][S][N]; every
  // split lies inside one segment of dp_seg_rows rows (host-aligned)
  const uint16_t* dY2;
  const float* dp_coef;
  int dp_seg_rows, dp_S;
  size_t slab_stride;  // floats between split slabs (N*K; 0 only in the attribution experiment)
  uint32_t x_step;     // wgrad_xp XLIN: X bytes per 64-row step (wgrad_x_linear)
};

// Weight-gradient MFMA shape: 16 = v_mfma_f32_16x16x32_bf16 (f32x4 accumulators), 32 =
// v_mfma_f32_32x32x16_bf16 (f32x16).  Same FLOPs and LDS fragment bytes per wave tile; the
// 32x32 form issues half the MFMA instructions and reads its operands as 32-column blocks.
template <int MF> struct WMfma;
template <> struct WMfma<16> { typedef f32x4 acc_t; };
template <> struct WMfma<32> { typedef f32x16 acc_t; };

// LDS swizzle of the weight-gradient operand images (XOR of 4-element units, 16-byte chunks kept
// whole).  MF 16: tr_swz (the transposed half-wave read covers rows q, q + 8 x 16 columns).
// MF 32: the half-wave read covers rows q = 0..3 x 32 columns (8 units = 16 banks): XOR the unit
// by (r & 3) << 3 so the four rows land on disjoint 16-bank quarters (rows of 128 / 256
// elements all start at bank 0).
template <int W, int MF>
__device__ __forceinline__ int wg_swz(int r, int col) {
  if constexpr (MF == 16) {
    return tr_swz<W>(r, col);
  } else {
    static_assert(W >= 128, "32x32 weight-gradient images need >= 32 units per row");
    return ((((col >> 2) ^ ((r & 3) << 3))) << 2) | (col & 3);
  }
}

// One 64-deep step of the weight-gradient tile from swizzled row-major LDS images (rows = m):
// both MFMA operands are read transposed with ds_read_b64_tr_b16.
template <int BCO, int BKK, int WM, int WN, int KS = 2, int MF = 16>
__device__ __forceinline__ void wgrad_mma(
    const uint16_t* Db, const uint16_t* Xb,
    typename WMfma<MF>::acc_t (&acc)[BCO / WM / MF][BKK / WN / MF]) {
  constexpr int TCO = BCO / WM, TKK = BKK / WN;
  constexpr int SD = BCO, SX = BKK;
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int wm = wid / WN, wn = wid % WN;
  const int g = lane >> 4, li = lane & 15, q = li >> 2, pp = li & 3;
  typedef short i16x8 __attribute__((ext_vector_type(8)));
  if constexpr (MF == 32) {
    // lane l holds A[row l & 31][k 8 (l >> 5) + j]: 16-lane group g reads the 4 x 16 block at
    // k rows 8 (g >> 1) + 0..3 (lo) / + 4..7 (hi), columns 16 (g & 1) + 0..15 of the fragment
    constexpr int FM = TCO / 32, FN = TKK / 32;
#pragma unroll
    for (int ks = 0; ks < 2 * KS; ++ks) {
      const int r1 = ks * 16 + 8 * (g >> 1) + q;
      bf16x8 af[FM], bfr[FN];
#pragma unroll
      for (int fm = 0; fm < FM; ++fm) {
        const int col = wm * TCO + fm * 32 + 16 * (g & 1) + 4 * pp;
        i16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
            LDS_PTR(i16x4, Db + r1 * SD + (wg_swz<BCO, 32>(r1, col))));
        i16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
            LDS_PTR(i16x4, Db + (r1 + 4) * SD + (wg_swz<BCO, 32>(r1 + 4, col))));
        i16x8 v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        af[fm] = __builtin_bit_cast(bf16x8, v);
      }
#pragma unroll
      for (int fn = 0; fn < FN; ++fn) {
        const int col = wn * TKK + fn * 32 + 16 * (g & 1) + 4 * pp;
        i16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
            LDS_PTR(i16x4, Xb + r1 * SX + (wg_swz<BKK, 32>(r1, col))));
        i16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
            LDS_PTR(i16x4, Xb + (r1 + 4) * SX + (wg_swz<BKK, 32>(r1 + 4, col))));
        i16x8 v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        bfr[fn] = __builtin_bit_cast(bf16x8, v);
      }
#pragma unroll
      for (int fm = 0; fm < FM; ++fm)
#pragma unroll
        for (int fn = 0; fn < FN; ++fn)
          acc[fm][fn] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[fm], bfr[fn], acc[fm][fn], 0, 0, 0);
    }
    return;
  } else {
  constexpr int FM = TCO / 16, FN = TKK / 16;
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    const int r1 = ks * 32 + 8 * g + q;
    bf16x8 af[FM], bfr[FN];
#pragma unroll
    for (int fm = 0; fm < FM; ++fm) {
      const int col = wm * TCO + fm * 16 + 4 * pp;
      i16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
          LDS_PTR(i16x4, Db + r1 * SD + tr_swz<BCO>(r1, col)));
      i16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
          LDS_PTR(i16x4, Db + (r1 + 4) * SD + tr_swz<BCO>(r1 + 4, col)));
      i16x8 v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
      af[fm] = __builtin_bit_cast(bf16x8, v);
    }
#pragma unroll
    for (int fn = 0; fn < FN; ++fn) {
      const int col = wn * TKK + fn * 16 + 4 * pp;
      i16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
          LDS_PTR(i16x4, Xb + r1 * SX + tr_swz<BKK>(r1, col)));
      i16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
          LDS_PTR(i16x4, Xb + (r1 + 4) * SX + tr_swz<BKK>(r1 + 4, col)));
      i16x8 v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
      bfr[fn] = __builtin_bit_cast(bf16x8, v);
    }
#pragma unroll
    for (int fm = 0; fm < FM; ++fm)
#pragma unroll
      for (int fn = 0; fn < FN; ++fn)
        acc[fm][fn] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[fm], bfr[fn], acc[fm][fn], 0, 0, 0);
  }
  }
}

// Sum of `cnt` float4 slabs `step` float4s apart (fixed order: four interleaved partial sums
// combined at the end, so four independent loads are in flight per thread instead of one
// dependent chain — the split reductions were latency-bound at ~20 us per call).
__device__ __forceinline__ float4 slab_sum4(const float4* __restrict__ p, size_t step, int cnt) {
  float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a, c = a, d = a;
  int sp = 0;
  for (; sp + 3 < cnt; sp += 4) {
    const float4 v0 = p[(size_t)sp * step], v1 = p[(size_t)(sp + 1) * step];
    const float4 v2 = p[(size_t)(sp + 2) * step], v3 = p[(size_t)(sp + 3) * step];
    a.x += v0.x; a.y += v0.y; a.z += v0.z; a.w += v0.w;
    b.x += v1.x; b.y += v1.y; b.z += v1.z; b.w += v1.w;
    c.x += v2.x; c.y += v2.y; c.z += v2.z; c.w += v2.w;
    d.x += v3.x; d.y += v3.y; d.z += v3.z; d.w += v3.w;
  }
  for (; sp < cnt; ++sp) {
    const float4 v = p[(size_t)sp * step];
    a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w;
  }
  return make_float4((a.x + b.x) + (c.x + d.x), (a.y + b.y) + (c.y + d.y),
                     (a.z + b.z) + (c.z + d.z), (a.w + b.w) + (c.w + d.w));
}


// fp32 partial slab of one split: partial[split][co][k], one wave's TCO x TKK tile at
// (cw, kw) (absolute output channel / K column of its first element)
template <int TCO, int TKK, int MF>
__device__ __forceinline__ void wgrad_store_at(
    const WgradArgs& p, typename WMfma<MF>::acc_t (&acc)[TCO / MF][TKK / MF], int split, int cw,
    int kw) {
  constexpr int FM = TCO / MF, FN = TKK / MF;
  const int lane = threadIdx.x & 63;
  const int g = lane >> 4, li = lane & 15;
  float* out = p.partial + (size_t)split * p.slab_stride;
  // a whole wave tile (the usual case) stores without per-element guards: the guarded loop
  // becomes one exec-mask branch per store (FM x FN x 16 of them per thread at 32x32)
  const bool full = cw + TCO <= p.N && kw + TKK <= p.K;
  if constexpr (MF == 32) {
    // D[row][col]: col = lane & 31, row = (i & 3) + 8 (i >> 2) + 4 (lane >> 5)
#pragma unroll
    for (int fm = 0; fm < FM; ++fm)
#pragma unroll
      for (int fn = 0; fn < FN; ++fn) {
        const int kcol = kw + fn * 32 + (lane & 31);
        const int cob = cw + fm * 32 + 4 * (lane >> 5);
        if (full) {
          float* o = out + (size_t)cob * p.K + kcol;
#pragma unroll
          for (int i = 0; i < 16; ++i) o[(size_t)((i & 3) + 8 * (i >> 2)) * p.K] = acc[fm][fn][i];
        } else {
#pragma unroll
          for (int i = 0; i < 16; ++i) {
            const int co = cob + (i & 3) + 8 * (i >> 2);
            if (co < p.N && kcol < p.K) out[(size_t)co * p.K + kcol] = acc[fm][fn][i];
          }
        }
      }
    return;
  }
#pragma unroll
  for (int fm = 0; fm < FM; ++fm)
#pragma unroll
    for (int fn = 0; fn < FN; ++fn) {
      const int kcol = kw + fn * 16 + li;
      const int cob = cw + fm * 16 + g * 4;
      if (full) {
        float* o = out + (size_t)cob * p.K + kcol;
#pragma unroll
        for (int i = 0; i < 4; ++i) o[(size_t)i * p.K] = acc[fm][fn][i];
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int co = cob + i;
          if (co < p.N && kcol < p.K) out[(size_t)co * p.K + kcol] = acc[fm][fn][i];
        }
      }
    }
}

template <int BCO, int BKK, int WM, int WN, int MF = 16>
__device__ __forceinline__ void wgrad_store(
    const WgradArgs& p, typename WMfma<MF>::acc_t (&acc)[BCO / WM / MF][BKK / WN / MF],
    int split, int co0, int k0) {
  const int wid = threadIdx.x >> 6;
  wgrad_store_at<BCO / WM, BKK / WN, MF>(p, acc, split, co0 + (wid / WN) * (BCO / WM),
                                         k0 + (wid % WN) * (BKK / WN));
}

template <class T, int FM, int FN>
__device__ __forceinline__ void zero_acc(T (&acc)[FM][FN]) {
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j) acc[i][j] = T{};
}

// A block's share of the weight gradient: the (co0, k0) corner of its BCO x BKK tile and rows
// [mbeg, mend) of its split, walked in nit steps of SR rows.  The host splits M in 64-row units;
// a trailing split may be empty (mend <= mbeg): it runs no step and stores a zero slab.
struct WgBlock {
  int split, co0, k0, mbeg, mend, nit;
};
template <int BCO, int BKK, int SR = 64>
__device__ __forceinline__ WgBlock wg_block(const WgradArgs& p) {
  const int lbid = xcd_remap(blockIdx.x, gridDim.x);
  const int tiles = p.nCo * p.nKk;
  WgBlock b;
  b.split = lbid / tiles;
  const int tile = lbid % tiles;
  b.co0 = (tile / p.nKk) * BCO;
  b.k0 = (tile % p.nKk) * BKK;
  b.mbeg = b.split * p.iters_per_split * 64;
  const int mend_raw = b.mbeg + p.iters_per_split * 64;
  b.mend = mend_raw < p.M ? mend_raw : p.M;
  b.nit = b.mend > b.mbeg ? (b.mend - b.mbeg + SR - 1) / SR : 0;
  return b;
}

// Incremental im2col addressing of NJ operand rows per thread: every row advances by exactly SR
// output pixels per step, so (n, oh, ow) are carried forward with compares instead of two integer
// divisions per chunk per step (those divisions were ~40 % of the loop's VALU work).
template <int NJ, int SR>
struct Im2colCursor {
  int n[NJ], oh[NJ], ow[NJ];
  int dn, doh, dow;  // SR rows as (images, output rows, output columns)
  __device__ __forceinline__ void init(const WgradArgs& p) {
    const int OHW = p.OH * p.OW;
    dn = SR / OHW;
    const int dr = SR - dn * OHW;
    doh = dr / p.OW;
    dow = dr - doh * p.OW;
  }
  __device__ __forceinline__ void seek(const WgradArgs& p, int j, int m) {
    const int OHW = p.OH * p.OW;
    n[j] = m / OHW;
    const int rem = m - n[j] * OHW;
    oh[j] = rem / p.OW;
    ow[j] = rem - oh[j] * p.OW;
  }
  // Byte offset of row j's 16-byte chunk at channel ci of the tap at (ihb, iwb).  ok: in, row and
  // column lie inside the problem; out, and the tap inside the image.  Where it does not hold the
  // offset is p.x_bytes, out of the buffer's range: the load returns zeros.
  // 24-bit multiplies (full-rate v_mul_u32_u24): every factor is < 2^24 and the byte offset
  // < 2^31 (host-checked), so the low 32 bits are exact
  __device__ __forceinline__ uint32_t x_off(const WgradArgs& p, int j, int ihb, int iwb, int ci,
                                            bool& ok) const {
    const int ih = (int)__umul24((unsigned)oh[j], (unsigned)p.ish) + ihb;
    const int iw = (int)__umul24((unsigned)ow[j], (unsigned)p.isw) + iwb;
    ok = ok && (unsigned)ih < (unsigned)p.IH && (unsigned)iw < (unsigned)p.IW;
    const uint32_t pix =
        __umul24(__umul24((unsigned)n[j], (unsigned)p.IH) + (unsigned)ih, (unsigned)p.IW) +
        (unsigned)iw;
    return ok ? __umul24(pix, (unsigned)(p.C * 2)) + (uint32_t)(ci * 2) : p.x_bytes;
  }
  __device__ __forceinline__ void advance(const WgradArgs& p, int j) {
    int w = ow[j] + dow, h = oh[j] + doh, i = n[j] + dn;
    if (w >= p.OW) { w -= p.OW; ++h; }
    if (h >= p.OH) { h -= p.OH; ++i; }
    ow[j] = w; oh[j] = h; n[j] = i;
  }
};

// dY operand of the LDS-DMA weight gradients (NW waves, steps of SR rows): lane → (row in piece,
// physical chunk) → the logical column chunk wg_swz maps onto that lane-linear LDS slot.
template <int BCO, int NW, int SR, int MF>
struct WgDyLane {
  static constexpr int CPD = BCO / 8, RPD = 64 / CPD, DI = SR / (RPD * NW);
  static_assert(DI >= 1 && DI * RPD * NW == SR, "wgrad dY lane mapping");
  int row[DI];
  uint32_t off[DI], dstep;
  bool cok[DI];
  __device__ __forceinline__ void init(const WgradArgs& p, const WgBlock& blk) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
    for (int j = 0; j < DI; ++j) {
      const int r = (j * NW + wid) * RPD + lane / CPD;
      const int col = blk.co0 + wg_swz<BCO, MF>(r, (lane % CPD) * 8);
      row[j] = r;
      cok[j] = col < p.N;
      off[j] = (uint32_t)(((size_t)(blk.mbeg + r) * p.N + col) * 2);
    }
    dstep = (uint32_t)(SR * p.N * 2);
  }
  // DMA of step `it` into stage `buf` of Ds ([stages][SR][BCO]); steps are issued in order
  __device__ __forceinline__ void issue(const WgradArgs& p, __amdgpu_buffer_rsrc_t rd,
                                        const uint16_t* Ds, int it, int buf, const WgBlock& blk) {
    const int wid = threadIdx.x >> 6;
    const int mb = blk.mbeg + it * SR;
#pragma unroll
    for (int j = 0; j < DI; ++j) {
      const bool ok = mb + row[j] < blk.mend && cok[j];
      dma16_opaque(rd, Ds + buf * SR * BCO + (j * NW + wid) * RPD * BCO, ok ? off[j] : p.dy_bytes);
      off[j] += dstep;
    }
  }
};

// im2col(X) operand of the same kernels: fixed (tap, channel) per lane and piece (the block's k
// window is fixed), output pixel carried incrementally.
template <int BKK, int NW, int SR, int MF>
struct WgXLane {
  static constexpr int CPX = BKK / 8, RPX = 64 / CPX, XI = SR / (RPX * NW);
  static_assert(XI >= 1 && XI * RPX * NW == SR, "wgrad X lane mapping");
  int row[XI], ci[XI], ihb[XI], iwb[XI];
  bool kok[XI];
  Im2colCursor<XI, SR> px;
  __device__ __forceinline__ void init(const WgradArgs& p, const WgBlock& blk) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
    for (int j = 0; j < XI; ++j) {
      const int r = (j * NW + wid) * RPX + lane / CPX;
      const int kk = blk.k0 + wg_swz<BKK, MF>(r, (lane % CPX) * 8);
      row[j] = r;
      kok[j] = kk < p.K;
      const int tap = kok[j] ? kk / p.C : 0;
      ci[j] = kk - tap * p.C;
      const int kh = tap / p.KW, kw = tap - (tap / p.KW) * p.KW;
      ihb[j] = p.ih0 + kh * p.dh;
      iwb[j] = p.iw0 + kw * p.dw;
      px.seek(p, j, blk.mbeg + r);
    }
    px.init(p);
  }
  // LDS slot of piece j in stage `buf` of Xs ([stages][SR][BKK])
  __device__ __forceinline__ const uint16_t* slot(const uint16_t* Xs, int buf, int j) const {
    return Xs + buf * SR * BKK + (j * NW + (threadIdx.x >> 6)) * RPX * BKK;
  }
  __device__ __forceinline__ void issue(const WgradArgs& p, __amdgpu_buffer_rsrc_t rx,
                                        const uint16_t* Xs, int it, int buf, const WgBlock& blk) {
    const int mb = blk.mbeg + it * SR;
#pragma unroll
    for (int j = 0; j < XI; ++j) {
      bool ok = mb + row[j] < blk.mend && kok[j];
      dma16_opaque(rx, slot(Xs, buf, j), px.x_off(p, j, ihb[j], iwb[j], ci[j], ok));
      px.advance(p, j);
    }
  }
};

// DEEP: operand loads run two 64-row steps ahead in two register sets (loop unrolled by two, every
// set index static).  With one set the loads of step it+1 have only step it's MFMAs (~0.4 µs at
// two waves per SIMD) to arrive, less than an L2 / MALL round trip under load: the layer3 3x3
// weight gradient measured MFMA-busy 23 % with 3.6 VALU per MFMA (r3 log).
template <int BCO, int BKK, int WM, int WN, bool PRO, bool DPRO, bool DEEP = false>
__global__ __launch_bounds__(256, (BCO * BKK > 128 * 128) ? 1 : 2) void wgrad_tn(WgradArgs p) {
  constexpr int TCO = BCO / WM, TKK = BKK / WN;
  constexpr int FM = TCO / 16, FN = TKK / 16;
  // LDS images: unpadded rows with an XOR swizzle of 4-element (8-byte) units per row, chosen so
  // that every ds_read_b64_tr_b16 half-wave (rows q and q+8, 4 units each) hits 64 distinct
  // banks (modelled, then SQ_LDS_BANK_CONFLICT: the padded layout measured 0.5 conflicts/access)
  constexpr int SD = BCO;       // LDS row stride (elements) of the dY tile
  constexpr int SX = BKK;       // of the X tile
  constexpr int CPD = BCO / 8, CPX = BKK / 8;
  constexpr int DCH = 64 * CPD / 256, XCH = 64 * CPX / 256;
  constexpr int RD = 256 / CPD, RX = 256 / CPX;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  uint16_t* Ds = (uint16_t*)smem;      // [2][64][SD]
  uint16_t* Xs = Ds + 2 * 64 * SD;     // [2][64][SX]

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int wm = wid / WN, wn = wid % WN;
  const WgBlock blk = wg_block<BCO, BKK>(p);
  const int split = blk.split, co0 = blk.co0, k0 = blk.k0;
  const int mbeg = blk.mbeg, mend = blk.mend, nit = blk.nit;

  const __amdgpu_buffer_rsrc_t rd_src = buf_rsrc(p.dY, p.dy_bytes);
  const __amdgpu_buffer_rsrc_t rx_src = buf_rsrc(p.X, p.x_bytes);

  // dY chunk owned by this thread
  const int dch = tid % CPD, drow = tid / CPD;
  const int dcol = co0 + dch * 8;
  const bool dcol_ok = dcol < p.N;
  // X chunk: fixed k per thread for the whole block
  const int xch = tid % CPX, xrow = tid / CPX;
  const int kk = k0 + xch * 8;
  const bool k_ok = kk < p.K;
  const int tap = k_ok ? kk / p.C : 0;
  const int ci = kk - tap * p.C;
  const int kh = tap / p.KW;
  const int kw = tap - kh * p.KW;

  struct Stage {
    u32x4 rd[DCH], rx[XCH], rd2[DCH];
    bool dok[DCH], xok[XCH], xseg[XCH], dseg[DCH];
  };
  Stage S0, S1;
  // dY prologue coefficients of the split's first segment and of the next one: with at most two
  // segments (views) a split may straddle the boundary, each dY row picks its set (host-checked:
  // dp_S <= 2, or every split inside one segment)
  float dA[8], dB[8], dD[8], dA1[8], dB1[8], dD1[8];
  const __amdgpu_buffer_rsrc_t rd2_src = buf_rsrc(DPRO ? p.dY2 : p.dY, p.dy_bytes);
  const int dseg0 = DPRO ? mbeg / p.dp_seg_rows : 0;
  const int dseg_next_row = (dseg0 + 1) * p.dp_seg_rows;  // first row of the next segment
  if (DPRO) {
    const int cc = dcol_ok ? dcol : 0;
    const int s1 = dseg0 + 1 < p.dp_S ? dseg0 + 1 : dseg0;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      dA[e] = p.dp_coef[dseg0 * p.N + cc + e];
      dB[e] = p.dp_coef[(p.dp_S + dseg0) * p.N + cc + e];
      dD[e] = p.dp_coef[(2 * p.dp_S + dseg0) * p.N + cc + e];
      dA1[e] = p.dp_coef[s1 * p.N + cc + e];
      dB1[e] = p.dp_coef[(p.dp_S + s1) * p.N + cc + e];
      dD1[e] = p.dp_coef[(2 * p.dp_S + s1) * p.N + cc + e];
    }
  }
  constexpr bool pro = PRO;
  float psc0[8], psh0[8], psc1[8], psh1[8];
  if (pro) {
    const int cc = k_ok ? ci : 0;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      psc0[e] = p.pro_sc[cc + e];
      psh0[e] = p.pro_sh[cc + e];
      psc1[e] = p.pro_S > 1 ? p.pro_sc[p.C + cc + e] : psc0[e];
      psh1[e] = p.pro_S > 1 ? p.pro_sh[p.C + cc + e] : psh0[e];
    }
  }

  const int ihb = p.ih0 + kh * p.dh, iwb = p.iw0 + kw * p.dw;
  Im2colCursor<XCH, 64> px;
  px.init(p);
#pragma unroll
  for (int j = 0; j < XCH; ++j) px.seek(p, j, mbeg + xrow + RX * j);
  uint32_t doff[DCH];
#pragma unroll
  for (int j = 0; j < DCH; ++j) doff[j] = (uint32_t)(((size_t)(mbeg + drow + RD * j) * p.N + dcol) * 2);
  const uint32_t dstep = (uint32_t)(64 * p.N * 2);

  auto gload = [&](int it, Stage& st) {
    const int mb = mbeg + it * 64;
#pragma unroll
    for (int j = 0; j < DCH; ++j) {
      const int m = mb + drow + RD * j;
      const bool ok = m < mend && dcol_ok;
      st.rd[j] = __builtin_amdgcn_raw_buffer_load_b128(rd_src, ok ? doff[j] : p.dy_bytes, 0, 0);
      if (DPRO) {
        st.rd2[j] = __builtin_amdgcn_raw_buffer_load_b128(rd2_src, ok ? doff[j] : p.dy_bytes, 0, 0);
        st.dok[j] = ok;
        st.dseg[j] = m >= dseg_next_row;
      }
      doff[j] += dstep;
    }
#pragma unroll
    for (int j = 0; j < XCH; ++j) {
      const int m = mb + xrow + RX * j;
      bool ok = m < mend && k_ok;
      const uint32_t off = px.x_off(p, j, ihb, iwb, ci, ok);
      st.xok[j] = ok;
      st.xseg[j] = pro && m >= p.pro_seg_rows;
      st.rx[j] = __builtin_amdgcn_raw_buffer_load_b128(rx_src, off, 0, 0);
      px.advance(p, j);
    }
  };
  auto lstore = [&](int buf, const Stage& st) {
#pragma unroll
    for (int j = 0; j < DCH; ++j)
      *(u32x4*)(Ds + buf * 64 * SD + (drow + RD * j) * SD + tr_swz<BCO>(drow + RD * j, dch * 8)) =
          DPRO ? (st.dseg[j] ? bnbwd8(st.rd[j], st.rd2[j], dA1, dB1, dD1, st.dok[j])
                             : bnbwd8(st.rd[j], st.rd2[j], dA, dB, dD, st.dok[j]))
               : st.rd[j];
#pragma unroll
    for (int j = 0; j < XCH; ++j) {
      u32x4 v = st.rx[j];
      if (pro)
        v = st.xseg[j] ? affine_relu8(v, psc1, psh1, st.xok[j], p.pro_relu != 0)
                       : affine_relu8(v, psc0, psh0, st.xok[j], p.pro_relu != 0);
      *(u32x4*)(Xs + buf * 64 * SX + (xrow + RX * j) * SX + tr_swz<BKK>(xrow + RX * j, xch * 8)) = v;
    }
  };

  f32x4 acc[FM][FN];
  zero_acc(acc);

  if (nit > 0) {
    gload(0, S0);
    lstore(0, S0);
  }
  if constexpr (!DEEP) {
    __syncthreads();
    for (int it = 0; it < nit; ++it) {
      const int cur = it & 1;
      if (it + 1 < nit) gload(it + 1, S0);
      wgrad_mma<BCO, BKK, WM, WN>(Ds + cur * 64 * SD, Xs + cur * 64 * SX, acc);
      if (it + 1 < nit) lstore(cur ^ 1, S0);
      __syncthreads();
    }
  } else {
    // entering an even step it: LDS buffer 0 holds step it, S1 step it + 1, S0 step it + 2
    if (nit > 1) gload(1, S1);
    if (nit > 2) gload(2, S0);
    __syncthreads();
    // raw barriers: __syncthreads() emits vmcnt(0), which would drain the loads of the step
    // two ahead (still in flight in the other register set) and reduce the pipeline to one
    // step; the LDS hazards need only the LDS counter (the compiler waits for each register
    // set's loads before the lstore that consumes it)
    for (int it = 0; it < nit; it += 2) {
      wgrad_mma<BCO, BKK, WM, WN>(Ds, Xs, acc);
      if (it + 1 < nit) lstore(1, S1);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      if (it + 3 < nit) gload(it + 3, S1);
      if (it + 1 >= nit) break;
      wgrad_mma<BCO, BKK, WM, WN>(Ds + 64 * SD, Xs + 64 * SX, acc);
      if (it + 2 < nit) lstore(0, S0);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      if (it + 4 < nit) gload(it + 4, S0);
    }
  }
  wgrad_store<BCO, BKK, WM, WN>(p, acc, split, co0, k0);
}

// Weight gradient with LDS-DMA staging (no operand prologue; C % 64 == 0): the dY and im2col(X)
// row tiles are DMA'd into the same swizzled row-major images wgrad_tn builds (each lane fetches
// the logical chunk tr_swz maps onto its lane-linear LDS slot), then read transposed by
// ds_read_b64_tr_b16.  Each block's (co0, k0) window is fixed, so every lane's X column (tap,
// channel) is constant and only its output pixel advances by 64 rows per step.
// PRO (unpadded 1x1 only, host-checked): the X operand's BatchNorm-apply + ReLU runs on the
// landed LDS tile (per-row segment, per-column channel), one extra barrier per step.
// NST LDS stages: with NST == 3 the DMA of step it+2 is issued while step it computes and a
// counted vmcnt keeps step it+1's DMA in flight across the barrier (raw s_barrier: hipcc's
// __syncthreads() would drain it with vmcnt(0)) — for the HBM-bound 1x1 weight gradients.
// WG_CUT (analysis builds only, tools/wgrad_cut.sh; 0 in the shipped build): 1 = no operand DMA
// inside the loop (MFMAs on stale tiles), 2 = no MFMAs (the DMA + barrier pipeline alone)
#ifndef WG_CUT
#define WG_CUT 0
#endif
template <int BCO, int BKK, int WM, int WN, bool PRO, int NST, int MF = 16>
__global__ __launch_bounds__(64 * WM * WN, 1) void wgrad_glds(WgradArgs p) {
  static_assert(NST == 2 || NST == 3, "wgrad_glds stages");
  constexpr int NW = WM * WN;
  typedef WgDyLane<BCO, NW, 64, MF> DL;
  typedef WgXLane<BKK, NW, 64, MF> XL;
  constexpr int CPX = XL::CPX;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  uint16_t* Ds = (uint16_t*)smem;   // [2][64][BCO]
  uint16_t* Xs = Ds + NST * 64 * BCO;  // [NST][64][BKK]
  float* Pt = (float*)(Xs + NST * 64 * BKK);  // PRO: [sc, sh][segment 0, 1][BKK] of this k window

  const int tid = threadIdx.x;
  const WgBlock blk = wg_block<BCO, BKK>(p);
  const int k0 = blk.k0, mbeg = blk.mbeg, nit = blk.nit;
  const __amdgpu_buffer_rsrc_t rd = buf_rsrc(p.dY, p.dy_bytes);
  const __amdgpu_buffer_rsrc_t rx = buf_rsrc(p.X, p.x_bytes);
  DL dl;
  XL xl;
  dl.init(p, blk);
  xl.init(p, blk);
  auto issue = [&](int it, int buf) {
    dl.issue(p, rd, Ds, it, buf, blk);
    xl.issue(p, rx, Xs, it, buf, blk);
  };

  typename WMfma<MF>::acc_t acc[BCO / WM / MF][BKK / WN / MF];
  zero_acc(acc);

  constexpr int PER = DL::DI + XL::XI;  // DMA instructions per wave per step
  if (PRO) {
    // the prologue's per-channel table is staged in LDS before any DMA is issued: an ordinary
    // global load consumed inside the loop would make hipcc drain the DMA queue (vmcnt(0))
    for (int i = tid; i < 4 * BKK; i += 64 * NW) {
      const int which = i / (2 * BKK), sg = (i / BKK) & 1, col = i % BKK;
      const int kk = k0 + col < p.K ? k0 + col : 0;
      const int sgs = p.pro_S > 1 ? sg : 0;
      Pt[i] = (which ? p.pro_sh : p.pro_sc)[sgs * p.C + kk];
    }
    __syncthreads();
  }
  constexpr int PXC = 64 * CPX / (64 * NW);  // X-prologue chunks per thread per step
  // the thread's chunks share their tr_swz key (row bits 0-3) when they are 16k rows apart;
  // the 32 table registers only where the accumulators leave room (256 x 256: 128 of them)
  constexpr bool HOIST = (64 * NW / CPX) % 16 == 0 && (BCO / WM) * (BKK / WN) / 64 <= 64;
  const int ptc = tid % CPX;                             // the thread's physical chunk
  float pro_sc0[8], pro_sh0[8], pro_sc1[8], pro_sh1[8];  // its logical column's tables
  if (PRO && HOIST) {
    const int col = wg_swz<BKK, MF>(tid / CPX, ptc * 8);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      pro_sc0[e] = Pt[col + e];
      pro_sc1[e] = Pt[BKK + col + e];
      pro_sh0[e] = Pt[2 * BKK + col + e];
      pro_sh1[e] = Pt[3 * BKK + col + e];
    }
  }
  if (nit > 0) issue(0, 0);
  if (NST == 3 && nit > 1) issue(1, 1);
  for (int it = 0; it < nit; ++it) {
    const int cur = NST == 3 ? it % 3 : (it & 1);
    if (NST == 3 && it + 1 < nit)
      asm volatile("s_waitcnt vmcnt(%0)" ::"n"(PER) : "memory");  // step it+1 stays in flight
    else
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();  // step it landed for every wave; buffer (it-1) % NST is free
    if (WG_CUT != 1 && NST > 1 && it + NST - 1 < nit) issue(it + NST - 1, (it + NST - 1) % NST);
    if (PRO && !HOIST) {
      // rows past mend hold zero dY, so whatever the transform makes of them contributes 0;
      // columns past K are dropped by the store
      const int mb = mbeg + it * 64;
#pragma unroll
      for (int i = 0; i < PXC; ++i) {
        const int c = tid + i * 64 * NW;
        const int row = c / CPX, pc = c % CPX;
        const int col = wg_swz<BKK, MF>(row, pc * 8);
        const int sg = (p.pro_S > 1 && mb + row >= p.pro_seg_rows) ? 1 : 0;
        const float4* ps = (const float4*)(Pt + sg * BKK + col);
        const float4* ph = (const float4*)(Pt + (2 + sg) * BKK + col);
        const float4 s0 = ps[0], s1 = ps[1], h0 = ph[0], h1 = ph[1];
        const float sc[8] = {s0.x, s0.y, s0.z, s0.w, s1.x, s1.y, s1.z, s1.w};
        const float sh[8] = {h0.x, h0.y, h0.z, h0.w, h1.x, h1.y, h1.z, h1.w};
        u32x4* q = (u32x4*)(Xs + cur * 64 * BKK + row * BKK + pc * 8);
        *q = affine_relu8(*q, sc, sh, true, p.pro_relu != 0);
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
    } else if (PRO) {
      // as above; here the thread's chunks sit in rows a multiple of
      // 16 apart, so they share one logical column (tr_swz keys on row bits 0-3) and the same
      // rows recur every step: the tables were loaded into registers once (pro_sc0 .. pro_sh1),
      // and a step that lies inside one segment picks its set with a uniform branch
      const int mb = mbeg + it * 64;
      const bool seg1 = p.pro_S > 1 && mb >= p.pro_seg_rows;
      const bool mixed = p.pro_S > 1 && mb < p.pro_seg_rows && mb + 64 > p.pro_seg_rows;
      const bool relu = p.pro_relu != 0;
#pragma unroll
      for (int i = 0; i < PXC; ++i) {
        const int row = (tid + i * 64 * NW) / CPX;
        u32x4* q = (u32x4*)(Xs + cur * 64 * BKK + row * BKK + ptc * 8);
        const u32x4 v = *q;
        if (mixed) {
          const bool sg = mb + row >= p.pro_seg_rows;
          float sc[8], sh[8];
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            sc[e] = sg ? pro_sc1[e] : pro_sc0[e];
            sh[e] = sg ? pro_sh1[e] : pro_sh0[e];
          }
          *q = affine_relu8(v, sc, sh, true, relu);
        } else if (seg1) {
          *q = affine_relu8(v, pro_sc1, pro_sh1, true, relu);
        } else {
          *q = affine_relu8(v, pro_sc0, pro_sh0, true, relu);
        }
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
    }
    if (WG_CUT != 2) wgrad_mma<BCO, BKK, WM, WN, 2, MF>(Ds + cur * 64 * BCO, Xs + cur * 64 * BKK, acc);
  }
  wgrad_store<BCO, BKK, WM, WN, MF>(p, acc, blk.split, blk.co0, k0);
}

// Weight-gradient fragments of one k sub-step (32 rows at MF 16, 16 rows at MF 32) of one wave
template <int TCO, int TKK, int MF>
struct WgKs {
  bf16x8 a[TCO / MF], b[TKK / MF];
};

template <int SD, int SX, int TCO, int TKK, int MF>
__device__ __forceinline__ void wg_read_ks(const uint16_t* Db, const uint16_t* Xb, int ks, int co_w,
                                           int kk_w, WgKs<TCO, TKK, MF>& f) {
  typedef short i16x8 __attribute__((ext_vector_type(8)));
  const int lane = threadIdx.x & 63;
  const int g = lane >> 4, li = lane & 15, q = li >> 2, pp = li & 3;
  // rows / columns as in wgrad_mma (ks counts 32-row sub-steps at MF 16, 16-row ones at MF 32)
  const int r1 = MF == 16 ? ks * 32 + 8 * g + q : ks * 16 + 8 * (g >> 1) + q;
  const int cg = MF == 16 ? 4 * pp : 16 * (g & 1) + 4 * pp;
#pragma unroll
  for (int fm = 0; fm < TCO / MF; ++fm) {
    const int col = co_w + fm * MF + cg;
    i16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
        LDS_PTR(i16x4, Db + r1 * SD + (wg_swz<SD, MF>(r1, col))));
    i16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
        LDS_PTR(i16x4, Db + (r1 + 4) * SD + (wg_swz<SD, MF>(r1 + 4, col))));
    i16x8 v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    f.a[fm] = __builtin_bit_cast(bf16x8, v);
  }
#pragma unroll
  for (int fn = 0; fn < TKK / MF; ++fn) {
    const int col = kk_w + fn * MF + cg;
    i16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
        LDS_PTR(i16x4, Xb + r1 * SX + (wg_swz<SX, MF>(r1, col))));
    i16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
        LDS_PTR(i16x4, Xb + (r1 + 4) * SX + (wg_swz<SX, MF>(r1 + 4, col))));
    i16x8 v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    f.b[fn] = __builtin_bit_cast(bf16x8, v);
  }
}

template <int TCO, int TKK, int MF>
__device__ __forceinline__ void wg_mma_ks(const WgKs<TCO, TKK, MF>& f,
                                          typename WMfma<MF>::acc_t (&acc)[TCO / MF][TKK / MF]) {
#pragma unroll
  for (int fm = 0; fm < TCO / MF; ++fm)
#pragma unroll
    for (int fn = 0; fn < TKK / MF; ++fn) {
      if constexpr (MF == 16)
        acc[fm][fn] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(f.a[fm], f.b[fn], acc[fm][fn], 0, 0, 0);
      else
        acc[fm][fn] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f.a[fm], f.b[fn], acc[fm][fn], 0, 0, 0);
    }
}

// LDS-DMA weight gradient with the fragment reads carried across the barrier (no operand
// prologues).  In wgrad_glds every wave starts a step with its fragment reads right after the
// barrier, so all waves of the CU wait on LDS together while the MFMA pipes idle (the compute half
// alone ran at ~55 % of the MFMA rate, r4 log).  Here the fragments roll through two register
// sets: sub-step j + 1 (one MFMA k-step) is read while sub-step j multiplies, and the last
// sub-step of step it multiplies after the barrier, under the reads of step it + 1's first
// sub-step — reads are always in flight under MFMAs, and only two sub-steps of fragments are
// live (the 256 x 256 tile fits without spilling).  The barrier also frees the step's buffer:
// the DMA of step it + 2 is issued right after it (2 LDS stages, one step of DMA in flight, as
// wgrad_glds).
//
// XLIN: every lane's X gather address advances by the same p.x_step per 64-row step with a fixed
// validity (wgrad_x_linear: a 1x1 stride-1 unpadded conv, whose X rows are the output rows, or
// an output image of OH*OW pixels dividing 64, whose rows keep their (oh, ow) and advance n).
// The general form re-derives (n, oh, ow, ih, iw) and the bounds for every DMA piece of every
// step: ~6 VALU per MFMA in the layer3 3x3 weight gradient (profiles/r6_wgrad_pmc.md).
template <int BCO, int BKK, int WM, int WN, int MF, bool XLIN = false>
__global__ __launch_bounds__(64 * WM * WN, 1) void wgrad_xp(WgradArgs p) {
  constexpr int NW = WM * WN;
  typedef WgDyLane<BCO, NW, 64, MF> DL;
  typedef WgXLane<BKK, NW, 64, MF> XL;
  constexpr int XI = XL::XI, PER = DL::DI + XI;
  constexpr int TCO = BCO / WM, TKK = BKK / WN;
  constexpr int NSUB = MF == 16 ? 2 : 4;  // k sub-steps per 64-row step (even: f[0] restarts)
  extern __shared__ __attribute__((aligned(16))) char smem[];
  uint16_t* Ds = (uint16_t*)smem;       // [2][64][BCO]
  uint16_t* Xs = Ds + 2 * 64 * BCO;     // [2][64][BKK]

  const int wid = threadIdx.x >> 6;
  const int co_w = (wid / WN) * TCO, kk_w = (wid % WN) * TKK;
  const WgBlock blk = wg_block<BCO, BKK>(p);
  const int nit = blk.nit;
  const __amdgpu_buffer_rsrc_t rd = buf_rsrc(p.dY, p.dy_bytes);
  const __amdgpu_buffer_rsrc_t rx = buf_rsrc(p.X, p.x_bytes);
  DL dl;
  XL xl;
  dl.init(p, blk);
  xl.init(p, blk);
  uint32_t xl_off[XLIN ? XI : 1];
  bool xl_ok[XLIN ? XI : 1];
  if constexpr (XLIN) {
    const int cstride = p.C * 2;
#pragma unroll
    for (int j = 0; j < XI; ++j) {
      const int ih = xl.px.oh[j] * p.ish + xl.ihb[j];
      const int iw = xl.px.ow[j] * p.isw + xl.iwb[j];
      xl_ok[j] = xl.kok[j] && (unsigned)ih < (unsigned)p.IH && (unsigned)iw < (unsigned)p.IW;
      xl_off[j] = xl_ok[j] ? (uint32_t)((((size_t)xl.px.n[j] * p.IH + ih) * p.IW + iw) * cstride +
                                        xl.ci[j] * 2)
                           : 0u;
    }
  }

  auto issue = [&](int it, int buf) {
    dl.issue(p, rd, Ds, it, buf, blk);
    if constexpr (XLIN) {
      const int mb = blk.mbeg + it * 64;
#pragma unroll
      for (int j = 0; j < XI; ++j) {
        const bool ok = mb + xl.row[j] < blk.mend && xl_ok[j];
        dma16_opaque(rx, xl.slot(Xs, buf, j), ok ? xl_off[j] : p.x_bytes);
        xl_off[j] += p.x_step;
      }
    } else {
      xl.issue(p, rx, Xs, it, buf, blk);
    }
  };

  typename WMfma<MF>::acc_t acc[TCO / MF][TKK / MF];
  zero_acc(acc);
  WgKs<TCO, TKK, MF> f[2];  // rolling pair: sub-step j + 1 is read while sub-step j multiplies

  if (nit > 0) {
    issue(0, 0);
    if (nit > 1) {
      issue(1, 1);
      asm volatile("s_waitcnt vmcnt(%0)" ::"n"(PER) : "memory");  // step 0 landed
    } else {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __builtin_amdgcn_s_barrier();
    wg_read_ks<BCO, BKK, TCO, TKK, MF>(Ds, Xs, 0, co_w, kk_w, f[0]);
  }
  for (int it = 0; it < nit; ++it) {
    const int cur = it & 1;
    const uint16_t* Db = Ds + cur * 64 * BCO;
    const uint16_t* Xb = Xs + cur * 64 * BKK;
#pragma unroll
    for (int j = 0; j < NSUB; ++j) {
      if (j + 1 < NSUB) {
        wg_read_ks<BCO, BKK, TCO, TKK, MF>(Db, Xb, j + 1, co_w, kk_w, f[(j + 1) & 1]);
      } else {
        // this wave's reads of step it retired; step it + 1 landed (nothing else in flight).
        // sched_barrier keeps the last sub-step's MFMAs below the barrier, under the next
        // step's first reads
        __builtin_amdgcn_sched_barrier(0);
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();  // every wave done with buffer cur; step it + 1 visible
        __builtin_amdgcn_sched_barrier(0);
        if (it + 2 < nit) issue(it + 2, cur);
        if (it + 1 < nit)
          wg_read_ks<BCO, BKK, TCO, TKK, MF>(Ds + (cur ^ 1) * 64 * BCO, Xs + (cur ^ 1) * 64 * BKK,
                                             0, co_w, kk_w, f[0]);
      }
      wg_mma_ks<TCO, TKK, MF>(f[j & 1], acc);
    }
  }
  wgrad_store_at<TCO, TKK, MF>(p, acc, blk.split, blk.co0 + co_w, blk.k0 + kk_w);
}

// Deep-pipelined LDS-DMA weight gradient (no operand prologues).  wgrad_glds stages 64-row
// steps in two LDS buffers: the DMA of step it+1 is issued at the top of step it and must land
// within ONE step of MFMAs (~0.4-0.9 us for the big tiles) — less than an HBM / remote-L2 round
// trip under load, so every step waited on its data (MFMA busy ~23 %, r3 optimisation log).
// Here a step is SR = 32 rows (one 16x16x32 MFMA k-step), the LDS holds NST steps and NST - 1 of
// them are in flight: the DMA of step it + NST - 1 is issued right after the barrier of step it,
// so it has NST - 1 steps of MFMAs to land.  A counted vmcnt keeps the later steps in flight
// across the raw barrier (never vmcnt(0) in the loop: cdna_hip_programming.md "Pipelining
// across barriers"); the barrier also publishes that every wave's fragment reads of the buffer
// being refilled have retired (lgkmcnt(0) before it).  s_setprio(1) around the MFMA cluster
// keeps hipcc from hoisting MFMAs across the barriers.
template <int BCO, int BKK, int WM, int WN, int SR, int NST, int MF = 16>
__global__ __launch_bounds__(64 * WM * WN, 1) void wgrad_pipe(WgradArgs p) {
  constexpr int NW = WM * WN;
  constexpr int CPD = BCO / 8, RPD = 64 / CPD, DI = SR / (RPD * NW);
  constexpr int CPX = BKK / 8, RPX = 64 / CPX, XI = SR / (RPX * NW);
  static_assert(SR % 32 == 0 && DI >= 1 && XI >= 1 && DI * RPD * NW == SR &&
                    XI * RPX * NW == SR, "wgrad pipe mapping");
  static_assert(NST >= 3 && NST <= 6, "wgrad pipe stages");
  constexpr int PER = DI + XI;  // DMA instructions per wave per step
  extern __shared__ __attribute__((aligned(16))) char smem[];
  uint16_t* Ds = (uint16_t*)smem;           // [NST][SR][BCO]
  uint16_t* Xs = Ds + NST * SR * BCO;       // [NST][SR][BKK]

  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int lbid = xcd_remap(blockIdx.x, gridDim.x);
  const int tiles = p.nCo * p.nKk;
  const int split = lbid / tiles;
  const int tile = lbid % tiles;
  const int co0 = (tile / p.nKk) * BCO;
  const int k0 = (tile % p.nKk) * BKK;
  const __amdgpu_buffer_rsrc_t rd = buf_rsrc(p.dY, p.dy_bytes);
  const __amdgpu_buffer_rsrc_t rx = buf_rsrc(p.X, p.x_bytes);
  const int mbeg = split * p.iters_per_split * 64;  // host splits in 64-row units
  const int mend_raw = mbeg + p.iters_per_split * 64;
  const int mend = mend_raw < p.M ? mend_raw : p.M;
  const int nit = mend > mbeg ? (mend - mbeg + SR - 1) / SR : 0;
  const int OHW = p.OH * p.OW;

  int d_row[DI];
  uint32_t d_off[DI];
  bool d_cok[DI];
#pragma unroll
  for (int j = 0; j < DI; ++j) {
    const int r = (j * NW + wid) * RPD + lane / CPD;
    const int col = co0 + wg_swz<BCO, MF>(r, (lane % CPD) * 8);
    d_row[j] = r;
    d_cok[j] = col < p.N;
    d_off[j] = (uint32_t)(((size_t)(mbeg + r) * p.N + col) * 2);
  }
  const uint32_t dstep = (uint32_t)(SR * p.N * 2);
  int x_row[XI], x_ci[XI], x_ihb[XI], x_iwb[XI], xn[XI], xoh[XI], xow[XI];
  bool x_kok[XI];
#pragma unroll
  for (int j = 0; j < XI; ++j) {
    const int r = (j * NW + wid) * RPX + lane / CPX;
    const int kk = k0 + wg_swz<BKK, MF>(r, (lane % CPX) * 8);
    x_row[j] = r;
    x_kok[j] = kk < p.K;
    const int tap = x_kok[j] ? kk / p.C : 0;
    x_ci[j] = kk - tap * p.C;
    const int kh = tap / p.KW, kw = tap - (tap / p.KW) * p.KW;
    x_ihb[j] = p.ih0 + kh * p.dh;
    x_iwb[j] = p.iw0 + kw * p.dw;
    const int m = mbeg + r;
    xn[j] = m / OHW;
    const int rem = m - xn[j] * OHW;
    xoh[j] = rem / p.OW;
    xow[j] = rem - xoh[j] * p.OW;
  }
  const int dn = SR / OHW, dr = SR - dn * OHW;
  const int doh = dr / p.OW, dow = dr - doh * p.OW;
  const int cstride = p.C * 2;

  auto issue = [&](int it, int buf) {
    const int mb = mbeg + it * SR;
#pragma unroll
    for (int j = 0; j < DI; ++j) {
      const bool ok = mb + d_row[j] < mend && d_cok[j];
      dma16_opaque(rd, Ds + buf * SR * BCO + (j * NW + wid) * RPD * BCO,
                   ok ? d_off[j] : p.dy_bytes);
      d_off[j] += dstep;
    }
#pragma unroll
    for (int j = 0; j < XI; ++j) {
      const int ih = (int)__umul24((unsigned)xoh[j], (unsigned)p.ish) + x_ihb[j];
      const int iw = (int)__umul24((unsigned)xow[j], (unsigned)p.isw) + x_iwb[j];
      const bool ok = mb + x_row[j] < mend && x_kok[j] && (unsigned)ih < (unsigned)p.IH &&
                      (unsigned)iw < (unsigned)p.IW;
      const uint32_t pix =
          __umul24(__umul24((unsigned)xn[j], (unsigned)p.IH) + (unsigned)ih, (unsigned)p.IW) +
          (unsigned)iw;
      const uint32_t off = ok ? __umul24(pix, (unsigned)cstride) + (uint32_t)(x_ci[j] * 2)
                              : p.x_bytes;
      dma16_opaque(rx, Xs + buf * SR * BKK + (j * NW + wid) * RPX * BKK, off);
      int ow = xow[j] + dow, oh = xoh[j] + doh, n = xn[j] + dn;
      if (ow >= p.OW) { ow -= p.OW; ++oh; }
      if (oh >= p.OH) { oh -= p.OH; ++n; }
      xow[j] = ow; xoh[j] = oh; xn[j] = n;
    }
  };

  typename WMfma<MF>::acc_t acc[BCO / WM / MF][BKK / WN / MF];
  zero_acc(acc);

#pragma unroll
  for (int j = 0; j < NST - 1; ++j)
    if (j < nit) issue(j, j);
  int cur = 0;
  for (int it = 0; it < nit; ++it) {
    // steps it+1 .. min(it+NST-2, nit-1) may stay in flight; step it must have landed
    const int ahead = min(NST - 2, nit - 1 - it);
    if (ahead >= NST - 2)
      asm volatile("s_waitcnt vmcnt(%0)" ::"n"(PER * (NST - 2)) : "memory");
    else if (NST > 3 && ahead == 2)
      asm volatile("s_waitcnt vmcnt(%0)" ::"n"(PER * 2) : "memory");
    else if (ahead == 1)
      asm volatile("s_waitcnt vmcnt(%0)" ::"n"(PER) : "memory");
    else
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();  // step it landed for every wave; buffer (it-1) % NST is free
    if (it + NST - 1 < nit) {
      const int nb = cur == 0 ? NST - 1 : cur - 1;  // (it + NST - 1) % NST
      issue(it + NST - 1, nb);
    }
    __builtin_amdgcn_s_setprio(1);
    wgrad_mma<BCO, BKK, WM, WN, SR / 32, MF>(Ds + cur * SR * BCO, Xs + cur * SR * BKK, acc);
    __builtin_amdgcn_s_setprio(0);
    cur = cur + 1 == NST ? 0 : cur + 1;
  }
  wgrad_store<BCO, BKK, WM, WN, MF>(p, acc, split, co0, k0);
}

// Weight gradient of a 3x3 / stride-1 / pad-1 convolution (16x16 / 32x32, C in {64, 128}) with
// the input patch reuse of igemm_patch: a block owns a (64 output channels, 64 input channels)
// tile of all 9 taps and walks its share of 256-pixel spatial tiles; per tile the dY rows and
// the halo'd input patch are DMA'd into LDS once (2 stages) and wave t (9 waves) accumulates tap
// t from them — the implicit GEMM's per-tap re-fetch of the input is gone.  Both operands are
// read with ds_read_b64_tr_b16 from tr_swz-swizzled images (patch rows = patch pixels, so the
// B rows of tap (kh, kw) are the pixels (r + kh, c + kw)).  iters_per_split counts 256-row tiles.
// Host guarantees (wgrad_variant_ok): igemm_patch_ok geometry, N % 64 == 0, no dY prologue;
// PRO: the X operand's BN-apply + ReLU on the landed patch (256-row tiles inside one segment).
#define TR_PTR(a) ((__attribute__((address_space(3))) i16x4*)(uintptr_t)(a))
template <bool PRO, int OW>
__global__ __launch_bounds__(576, 1) void wgrad_patch(WgradArgs p) {
  constexpr int B = 64;  // co and ci tile
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int C = p.C;
  constexpr int LG = OW == 32 ? 5 : 4, lg = LG;
  constexpr int TR = 256 / OW, PW = OW + 2, PP = (TR + 2) * PW;
  const int pinstr = (PP + 7) / 8;                 // 8 patch pixels (128 B each) per DMA
  const int stage = 256 * B + pinstr * 512;        // elements per stage: dY tile + patch
  uint16_t* S0 = (uint16_t*)smem;

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;  // wave = tap
  const int lbid = xcd_remap(blockIdx.x, gridDim.x);
  const int nci = C / B;
  const int tiles = p.nCo * nci;
  const int split = lbid / tiles;
  const int tile = lbid % tiles;
  const int co0 = (tile / nci) * B, ci0 = (tile % nci) * B;
  const int ntot = p.M / 256;
  const int t_beg = split * p.iters_per_split;
  const int t_end = min(ntot, t_beg + p.iters_per_split);
  const int OHW = p.OH * OW;
  const __amdgpu_buffer_rsrc_t rd = buf_rsrc(p.dY, p.dy_bytes);
  const __amdgpu_buffer_rsrc_t rx = buf_rsrc(p.X, p.x_bytes);
  const int lr = lane >> 3, lpc = lane & 7;

  auto issue = [&](int t, int buf) {
    uint16_t* D = S0 + buf * stage;
    uint16_t* P = D + 256 * B;
    const int img = (t * 256) / OHW;
    const int row0 = (t * 256 - img * OHW) >> lg;
    for (int i = wid; i < 32; i += 9) {  // dY: 8 rows x 128 B per instruction
      const int r = i * 8 + lr;
      const int col = co0 + tr_swz<B>(r, lpc * 8);
      dma16_opaque(rd, D + i * 512, (uint32_t)(((size_t)(t * 256 + r) * p.N + col) * 2));
    }
    for (int i = wid; i < pinstr; i += 9) {  // patch: 8 pixels x 128 B per instruction
      const int q = i * 8 + lr;
      const int ci = ci0 + tr_swz<B>(q, lpc * 8);
      const int pr = q / PW, pc = q - (q / PW) * PW;
      const int ih = row0 - 1 + pr, iw = pc - 1;
      const bool ok = q < PP && (unsigned)ih < (unsigned)p.IH && (unsigned)iw < (unsigned)p.IW;
      dma16_opaque(rx, P + i * 512,
            ok ? (uint32_t)((((img * p.IH + ih) * p.IW + iw) * C + ci) * 2) : p.x_bytes);
    }
  };

  f32x4 acc[4][4];
  zero_acc(acc);
  // PRO: the [S<=2][sc, sh][64] table of this block's input-channel slice, staged in LDS behind
  // the two stages BEFORE any DMA (global loads consumed inside the loop would make hipcc drain
  // the in-flight opaque DMA with vmcnt(0); tools/isa_check.py)
  float* Tb = (float*)(S0 + 2 * stage);
  if (PRO) {
    for (int i = tid; i < 2 * 2 * B; i += 576) {
      const int sg = i / (2 * B), k = (i / B) & 1, j = i % B;
      Tb[i] = sg < p.pro_S ? (k ? p.pro_sh : p.pro_sc)[sg * C + ci0 + j] : 0.f;
    }
    __syncthreads();
  }
  const int kh = wid / 3, kw = wid - (wid / 3) * 3;
  const int g = lane >> 4, li = lane & 15, qq = li >> 2, pp = li & 3;
  typedef short i16x8 __attribute__((ext_vector_type(8)));
  // Fragment byte offsets within a stage, fixed for every tile and k-step.  A lane's two row
  // reads (h = 0, 1) are tile rows ks·32 + o, o = 8g + qq + 4h.  tr_swz<64> of row r and column
  // 16f + 4pp is chunk (f ^ key(r))·32 + pp·8 bytes, key(r) from r's bits 1 and 3, so
  //   dY: r·128 + (f ^ key)·32 + pp·8 = ks·4096 + [o·128 + pp·8 + key(o)·32] ^ (f·32)
  //   patch: pixel q = qb + ks·DQ (DQ = PW, or 2·PW at OW 16): q·128 + ... with the key of the
  //   shifted pixel, kept as a 2-bit-per-k-step table — instead of ~90 VALU of index math per
  //   k-step (5-6 per MFMA, the loop's real limit) it is ~16.
  constexpr int DQ = OW == 32 ? PW : 2 * PW;
  const uint32_t lds0 = (uint32_t)(uintptr_t)LDS_PTR(const void, smem);
  uint32_t dv[2], pv[2], kmask[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int o = 8 * g + qq + 4 * h;
    const int kd = ((o >> 1) & 1) ^ (((o >> 3) & 1) << 1);
    dv[h] = (uint32_t)(o * 128 + pp * 8 + kd * 32);
    const int qb = ((o >> LG) + kh) * PW + (o & (OW - 1)) + kw;
    pv[h] = (uint32_t)(qb * 128 + pp * 8);
    uint32_t km = 0;
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) {
      const int q = qb + ks * DQ;
      km |= (uint32_t)(((q >> 1) & 1) ^ (((q >> 3) & 1) << 1)) << (2 * ks);
    }
    kmask[h] = km;
  }
  if (t_beg < t_end) issue(t_beg, 0);
  for (int t = t_beg; t < t_end; ++t) {
    const int cur = (t - t_beg) & 1;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (t + 1 < t_end) issue(t + 1, cur ^ 1);
    if (PRO) {
      // X operand = relu(bn(x)) of the conv's input, formed on the landed patch (the opaque
      // DMA of tile t+1 into the other stage stays in flight); padding pixels stay zero
      uint16_t* Pm = S0 + cur * stage + 256 * B;
      const int img = (t * 256) / OHW;
      const int row0 = (t * 256 - img * OHW) >> lg;
      const int pseg = (t * 256) / p.pro_seg_rows;  // tiles never straddle a segment (host)
      // the first 512 threads walk the patch 64 pixels apart: q & 63 stays fixed per thread, so
      // does the tr_swz-mapped channel chunk of its slot (the swizzle keys on row bits 1 and 3)
      // — its 8 scale / shift pairs come from the LDS table once per tile, the pixel walk is
      // incremental, and four chunks' LDS reads are issued before the first write-back
      if (tid < 512) {
        const int q0 = tid >> 3, pc8 = tid & 7;
        const int ch = tr_swz<B>(q0, pc8 * 8);  // within the block's 64-channel slice
        const float4* ps = (const float4*)(Tb + pseg * 2 * B + ch);
        const float4* ph = (const float4*)(Tb + pseg * 2 * B + B + ch);
        const float4 s0 = ps[0], s1 = ps[1], h0 = ph[0], h1 = ph[1];
        const f32x2 sc[4] = {{s0.x, s0.y}, {s0.z, s0.w}, {s1.x, s1.y}, {s1.z, s1.w}};
        const f32x2 sh[4] = {{h0.x, h0.y}, {h0.z, h0.w}, {h1.x, h1.y}, {h1.z, h1.w}};
        const int dr = 64 / PW, dc = 64 - dr * PW;
        int pr = q0 / PW, pc = q0 - pr * PW;
        uint16_t* base = Pm + tid * 8;  // chunk i at base + i·512·8
        const bool relu = p.pro_relu != 0;
        // two chunks per batch: this 9-wave kernel runs at the 170-VGPR cap of 3 waves / SIMD
        for (int i0 = 0; i0 * 64 + q0 < PP; i0 += 2) {
          u32x4 v[2];
          bool ok[2];
#pragma unroll
          for (int u = 0; u < 2; ++u) {
            const int ih = row0 - 1 + pr, iw = pc - 1;
            ok[u] = (i0 + u) * 64 + q0 < PP && (unsigned)ih < (unsigned)p.IH &&
                    (unsigned)iw < (unsigned)p.IW;
            if (ok[u]) v[u] = *(const u32x4*)(base + (i0 + u) * 4096);
            pr += dr;
            pc += dc;
            if (pc >= PW) { pc -= PW; ++pr; }
          }
#pragma unroll
          for (int u = 0; u < 2; ++u)
            if (ok[u]) *(u32x4*)(base + (i0 + u) * 4096) = affine_relu8_pk(v[u], sc, sh, relu);
        }
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
    }
    // this stage's LDS byte address (a multiple of 1 KiB: it leaves the swizzle bits 5-6 of the
    // fragment offsets alone, so base + (v ^ c) == (base + v) ^ c)
    const uint32_t sb = lds0 + (uint32_t)(cur * stage * 2);
    uint32_t dvt[2], pvt[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      dvt[h] = sb + dv[h];
      pvt[h] = sb + pv[h];
    }
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) {
      bf16x8 af[4], bfr[4];
      // dY rows ks·32 + o: ks·4096 B is an immediate; fragment fm sits at chunk (fm ^ key)
#pragma unroll
      for (int fm = 0; fm < 4; ++fm) {
        i16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
            TR_PTR((dvt[0] ^ (uint32_t)(fm * 32)) + (uint32_t)(ks * 4096)));
        i16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
            TR_PTR((dvt[1] ^ (uint32_t)(fm * 32)) + (uint32_t)(ks * 4096)));
        i16x8 v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        af[fm] = __builtin_bit_cast(bf16x8, v);
      }
      // patch pixels qb + ks·DQ: the shift is an immediate, the swizzle key of the shifted pixel
      // comes from the per-lane 2-bit table
      uint32_t pk[2];
#pragma unroll
      for (int h = 0; h < 2; ++h) pk[h] = pvt[h] | (((kmask[h] >> (2 * ks)) & 3u) << 5);
#pragma unroll
      for (int fn = 0; fn < 4; ++fn) {
        i16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
            TR_PTR((pk[0] ^ (uint32_t)(fn * 32)) + (uint32_t)(32768 + ks * DQ * 128)));
        i16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
            TR_PTR((pk[1] ^ (uint32_t)(fn * 32)) + (uint32_t)(32768 + ks * DQ * 128)));
        i16x8 v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        bfr[fn] = __builtin_bit_cast(bf16x8, v);
      }
#pragma unroll
      for (int fm = 0; fm < 4; ++fm)
#pragma unroll
        for (int fn = 0; fn < 4; ++fn)
          acc[fm][fn] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[fm], bfr[fn], acc[fm][fn], 0, 0, 0);
    }
  }
  // partial[split][co][tap * C + ci]
  float* out = p.partial + (size_t)split * p.slab_stride;
#pragma unroll
  for (int fm = 0; fm < 4; ++fm)
#pragma unroll
    for (int fn = 0; fn < 4; ++fn) {
      const int kcol = wid * C + ci0 + fn * 16 + li;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int co = co0 + fm * 16 + g * 4 + i;
        out[(size_t)co * p.K + kcol] = acc[fm][fn][i];
      }
    }
}

// out[co][tap][ci < Creal] (+)= Σ_s partial[s*stride][co][tap*C + ci]   (slab stride in slabs)
__global__ void wgrad_reduce(const float* __restrict__ partial, float* __restrict__ out, int splits,
                             int sstride, int N, int K, int C, int Creal, float beta) {
  const int taps = K / C;
  const size_t total = (size_t)N * taps * Creal;
  for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
       idx += (size_t)gridDim.x * blockDim.x) {
    const int ci = (int)(idx % Creal);
    const size_t t = idx / Creal;
    const int tap = (int)(t % taps);
    const int co = (int)(t / taps);
    const size_t src = (size_t)co * K + tap * C + ci;
    float s = 0.f;
    for (int sp = 0; sp < splits; ++sp) s += partial[(size_t)sp * sstride * N * K + src];
    out[idx] = beta != 0.f ? beta * out[idx] + s : s;
  }
}

__global__ void wgrad_reduce_vec4(const float4* __restrict__ partial, float4* __restrict__ out,
                                  int splits, int sstride, size_t n4, float beta) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4;
       i += (size_t)gridDim.x * blockDim.x) {
    float4 s = slab_sum4(partial + i, (size_t)sstride * n4, splits);
    if (beta != 0.f) {
      const float4 o = out[i];
      s.x += beta * o.x; s.y += beta * o.y; s.z += beta * o.z; s.w += beta * o.w;
    }
    out[i] = s;
  }
}
// In place: slab[i] = Σ_sp slab[sp * step + i] (channel-padded weight gradients reduce into
// slab 0 before the compaction).  No __restrict__: the output aliases the first slab; each
// element is read and written by the same thread.
__global__ void wgrad_reduce_vec4_inplace(float4* slab, int splits, int sstride, size_t n4) {
  const size_t step = (size_t)sstride * n4;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4;
       i += (size_t)gridDim.x * blockDim.x) {
    float4 a = slab[i];
    for (int sp = 1; sp < splits; ++sp) {
      const float4 v = slab[(size_t)sp * step + i];
      a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w;
    }
    slab[i] = a;
  }
}
// Small outputs with many splits (e.g. a 64 x 64 1x1 weight gradient split ~250 ways over 2^20
// rows): the two-level reduction gave each level a few blocks of long per-thread slab walks
// (67 µs at the very end of the step).  One launch instead: a block owns 16 float4 columns and
// spreads the slabs over 16 lanes (each thread sums every 16th slab, four loads in flight),
// then the lanes are combined through LDS in a fixed order (deterministic).
constexpr int RC_COLS = 16, RC_LANES = 16;
__global__ __launch_bounds__(256) void wgrad_reduce_cols(const float4* __restrict__ partial,
                                                         float4* __restrict__ out, int splits,
                                                         size_t n4, float beta) {
  __shared__ float4 red[RC_LANES][RC_COLS];
  const int col = threadIdx.x % RC_COLS, lane = threadIdx.x / RC_COLS;
  const size_t i = (size_t)blockIdx.x * RC_COLS + col;
  float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a, c = a, d = a;
  if (i < n4) {
    int sp = lane;
    for (; sp + 3 * RC_LANES < splits; sp += 4 * RC_LANES) {
      const float4 v0 = partial[(size_t)sp * n4 + i];
      const float4 v1 = partial[(size_t)(sp + RC_LANES) * n4 + i];
      const float4 v2 = partial[(size_t)(sp + 2 * RC_LANES) * n4 + i];
      const float4 v3 = partial[(size_t)(sp + 3 * RC_LANES) * n4 + i];
      a.x += v0.x; a.y += v0.y; a.z += v0.z; a.w += v0.w;
      b.x += v1.x; b.y += v1.y; b.z += v1.z; b.w += v1.w;
      c.x += v2.x; c.y += v2.y; c.z += v2.z; c.w += v2.w;
      d.x += v3.x; d.y += v3.y; d.z += v3.z; d.w += v3.w;
    }
    for (; sp < splits; sp += RC_LANES) {
      const float4 v = partial[(size_t)sp * n4 + i];
      a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w;
    }
  }
  red[lane][col] = make_float4((a.x + b.x) + (c.x + d.x), (a.y + b.y) + (c.y + d.y),
                               (a.z + b.z) + (c.z + d.z), (a.w + b.w) + (c.w + d.w));
  __syncthreads();
  if (lane == 0 && i < n4) {
    float4 s = red[0][col];
#pragma unroll
    for (int l = 1; l < RC_LANES; ++l) {
      const float4 v = red[l][col];
      s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
    }
    if (beta != 0.f) {
      const float4 o = out[i];
      s.x += beta * o.x; s.y += beta * o.y; s.z += beta * o.z; s.w += beta * o.w;
    }
    out[i] = s;
  }
}
// the column-parallel form pays where the two-level one has too few blocks
inline bool reduce_cols_ok(size_t n4, int splits) { return n4 <= 16384 && splits >= 32; }

__global__ void wgrad_reduce_l1(float4* __restrict__ partial, int splits, int group, size_t n4) {
  const int g = blockIdx.y;
  const int s0 = g * group;
  const int s1 = min(splits, s0 + group);
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4;
       i += (size_t)gridDim.x * blockDim.x) {
    partial[(size_t)s0 * n4 + i] = slab_sum4(partial + (size_t)s0 * n4 + i, n4, s1 - s0);
  }
}

// Wt[ci][khs][kws][co] = W[co][kh0 + khs*sh][kw0 + kws*sw][ci]   (bf16)
__global__ void weight_transform(const uint16_t* __restrict__ W, uint16_t* __restrict__ Wt,
                                 int Co, int KH, int KW, int Ci, int KHs, int KWs, int kh0, int sh,
                                 int kw0, int sw) {
  const size_t total = (size_t)Ci * KHs * KWs * Co;
  for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
       idx += (size_t)gridDim.x * blockDim.x) {
    const int co = (int)(idx % Co);
    size_t t = idx / Co;
    const int kws = (int)(t % KWs);
    t /= KWs;
    const int khs = (int)(t % KHs);
    const int ci = (int)(t / KHs);
    const int kh = kh0 + khs * sh, kw = kw0 + kws * sw;
    Wt[idx] = W[(((size_t)co * KH + kh) * KW + kw) * Ci + ci];
  }
}

// All dgrad weight transforms of a step in one launch: a table of WtDesc (built once per weight
// set, kernels.h), blocks assigned contiguously per descriptor and found by binary search.
// The weights change only at the optimizer step, so the ~60 per-conv launches collapse into
// one.  Each block transposes one 64(co) x 64(ci) tile of one (khs, kws) tap through LDS, so
// both the W reads (along ci) and the Wt writes (along co) are coalesced.
__global__ __launch_bounds__(256) void weight_transform_batch(const WtDesc* __restrict__ d, int n) {
  __shared__ uint16_t tile[64][65];
  int lo = 0, hi = n - 1;
  const int b = blockIdx.x;
  while (lo < hi) {  // last descriptor with blk0 <= b
    const int mid = (lo + hi + 1) >> 1;
    if (d[mid].blk0 <= b) lo = mid; else hi = mid - 1;
  }
  const WtDesc q = d[lo];
  const int nco = (q.Co + 63) / 64, nci = (q.Ci + 63) / 64;
  int t = b - q.blk0;
  const int tco = t % nco;
  t /= nco;
  const int tci = t % nci;
  t /= nci;
  const int kws = t % q.KWs, khs = t / q.KWs;
  const int kh = q.kh0 + khs * q.sh, kw = q.kw0 + kws * q.sw;
  const int co0 = tco * 64, ci0 = tci * 64;
#pragma unroll 4
  for (int e = 0; e < 16; ++e) {
    const int idx = threadIdx.x + 256 * e;
    const int r = idx >> 6, c = idx & 63;  // r: co, c: ci (consecutive threads along ci)
    const int co = co0 + r, ci = ci0 + c;
    if (co < q.Co && ci < q.Ci) tile[r][c] = q.W[(((size_t)co * q.KH + kh) * q.KW + kw) * q.Ci + ci];
  }
  __syncthreads();
#pragma unroll 4
  for (int e = 0; e < 16; ++e) {
    const int idx = threadIdx.x + 256 * e;
    const int r = idx >> 6, c = idx & 63;  // r: ci, c: co (consecutive threads along co)
    const int ci = ci0 + r, co = co0 + c;
    if (co < q.Co && ci < q.Ci)
      q.Wt[(((size_t)ci * q.KHs + khs) * q.KWs + kws) * q.Co + co] = tile[c][r];
  }
}

template <int BM, int BN, int WM, int WN, int PRO, int EPI>
void launch_igemm_t(const IgemmArgs& a0, hipStream_t s) {
  IgemmArgs a = a0;
  a.nMb = (a.M + BM - 1) / BM;
  a.nNb = (a.N + BN - 1) / BN;
  const int grid = a.nMb * a.nNb;
  size_t lds = (size_t)(a.K > 64 ? 2 : 1) * (BM + BN) * 64 * 2;
  const size_t cst = (size_t)BM * (BN + 8) * 2;
  const size_t red = (size_t)(256 / (BN / 8)) * BN * 3 * 4;
  if (cst > lds) lds = cst;
  if (red > lds) lds = red;
  hipLaunchKernelGGL((igemm_nt<BM, BN, WM, WN, PRO, EPI>), dim3(grid), dim3(256), lds, s, a);
  HIP_CHECK_LAUNCH();
}

template <int BM, int BN, int WM, int WN, int PRO, int EPI, int NST>
void launch_glds_t(const IgemmArgs& a0, hipStream_t s) {
  IgemmArgs a = a0;
  a.nMb = (a.M + BM - 1) / BM;
  a.nNb = (a.N + BN - 1) / BN;
  constexpr int NT = 64 * WM * WN;
  const size_t lds = igemm_glds_pro_offset(BM, BN, NT, a.K > 64 ? NST : 1, PRO >= 2 ? 2 : 1) +
                     (PRO ? (size_t)(PRO == 3 ? 4 : PRO == 2 ? 3 : 2) * a.C * 4 : 0);
  hipLaunchKernelGGL((igemm_glds<BM, BN, WM, WN, PRO, EPI, NST>), dim3(a.nMb * a.nNb), dim3(NT),
                     lds, s, a);
  HIP_CHECK_LAUNCH();
}

size_t igemm_patch_lds(int BN, int NT, int OW, int C) {
  const int ppi = 64 / (C / 8), pp = (256 / OW + 2) * (OW + 2);
  const size_t patch = (size_t)((pp + ppi - 1) / ppi) * 1024 + (size_t)2 * BN * 64 * 2;
  const size_t cst = (size_t)256 * (BN + 8) * 2;
  const size_t red = (size_t)(NT / (BN / 8)) * BN * 3 * 4;
  return std::max(patch, std::max(cst, red));
}

template <int BN, int WM, int WN, int EPI, int PRO = 0>
void launch_patch_t(const IgemmArgs& a0, hipStream_t s) {
  IgemmArgs a = a0;
  a.nMb = (a.M + 255) / 256;
  a.nNb = (a.N + BN - 1) / BN;
  constexpr int NT = 64 * WM * WN;
  hipLaunchKernelGGL((igemm_patch<BN, WM, WN, EPI, PRO>), dim3(a.nMb * a.nNb), dim3(NT),
                     igemm_patch_lds(BN, NT, a.OW, a.C), s, a);
  HIP_CHECK_LAUNCH();
}

// ---- compile-time fusion modes (prologue x epilogue), so each launch carries only its own work
// PRO: 0 none, 1 BN-apply, 2 BN-backward, 3 block-output.  EPI: epi_mode, 5 = mode 4 with the
// second BN stream.  igemm_fusion_allowed is the set of pairs a kernel family instantiates for a
// tile; the launchers and the host admissibility (igemm_variant_ok / igemm_dual_ok) both read it.
enum IgFam { IG_NT, IG_GLDS, IG_PATCH };  // register-staged igemm_nt, LDS-DMA igemm_glds, igemm_patch
constexpr int kNumPro = 4, kNumEpi = 6;
constexpr bool igemm_fusion_allowed(IgFam fam, int pro, int epi, int area, int stages) {
  if (pro == 0) return true;                  // every epilogue
  const bool bwd = epi == 0 || epi == 3;      // what every BN-backward prologue has
  switch (fam) {
    case IG_NT:  // BN-apply: no mode 4; no block-output prologue
      return pro == 1 ? epi <= 3 : pro == 2 && (bwd || epi >= 4);
    case IG_GLDS:
      // the 3-stage tiles leave no LDS for the prologue table; the single-stage ones have the
      // BN-apply prologue only; the block-output prologue takes the plain epilogue; a tile above
      // 256 x 128 with the BN-backward prologue and mode 4 drains its DMA pipeline
      if (pro == 1) return stages <= 2 && epi <= 3;
      if (stages != 2) return false;
      return pro == 2 ? bwd || (epi >= 4 && area <= 256 * 128) : epi == 0;
    case IG_PATCH:  // prologues on the landed patch: BN-apply with any epilogue
      return pro == 1 || (pro == 2 && bwd);
  }
  return false;
}
inline int igemm_pro_code(bool bn_apply, bool bn_bwd, bool block_out) {
  return bn_bwd ? 2 : block_out ? 3 : bn_apply ? 1 : 0;
}

template <IgFam FAM, int AREA, int STAGES, int I, class F>
bool launch_fusion_if(int pro, int epi, const IgemmArgs& a, hipStream_t s, F f) {
  constexpr int PRO = I / kNumEpi, EPI = I % kNumEpi;
  if constexpr (igemm_fusion_allowed(FAM, PRO, EPI, AREA, STAGES)) {
    if (pro == PRO && epi == EPI) {
      f(std::integral_constant<int, PRO>{}, std::integral_constant<int, EPI>{}, a, s);
      return true;
    }
  }
  return false;
}
// launch f(PRO, EPI, a, s) with the pair these arguments ask for
template <IgFam FAM, int AREA, int STAGES, class F, int... I>
void launch_fusion(const IgemmArgs& a, hipStream_t s, F f, std::integer_sequence<int, I...>) {
  const int pro = igemm_pro_code(a.pro_sc != nullptr, a.pro_d != nullptr, a.pro_out != nullptr);
  const int epi = a.epi_mode == 4 && a.stats2 != nullptr ? 5
                  : a.epi_mode >= 1 && a.epi_mode <= 4   ? a.epi_mode
                                                         : 0;
  if (!(launch_fusion_if<FAM, AREA, STAGES, I>(pro, epi, a, s, f) || ...)) {
    fprintf(stderr, "igemm: unsupported fusion (prologue %d, epilogue %d) on this tile\n", pro, epi);
    abort();  // the bindings reject this
  }
}
constexpr std::make_integer_sequence<int, kNumPro * kNumEpi> kFusionPairs{};

template <int BM, int BN, int WM, int WN>
void launch_igemm(const IgemmArgs& a, hipStream_t s) {
  launch_fusion<IG_NT, BM * BN, 2>(a, s, [](auto pro, auto epi, const IgemmArgs& a, hipStream_t s) {
    launch_igemm_t<BM, BN, WM, WN, decltype(pro)::value, decltype(epi)::value>(a, s);
  }, kFusionPairs);
}

template <int BM, int BN, int WM, int WN, int NST = 2>
void launch_glds(const IgemmArgs& a, hipStream_t s) {
  launch_fusion<IG_GLDS, BM * BN, NST>(a, s, [](auto pro, auto epi, const IgemmArgs& a, hipStream_t s) {
    launch_glds_t<BM, BN, WM, WN, decltype(pro)::value, decltype(epi)::value, NST>(a, s);
  }, kFusionPairs);
}

template <int BN, int WM, int WN>
void launch_patch(const IgemmArgs& a, hipStream_t s) {
  launch_fusion<IG_PATCH, 256 * BN, 2>(a, s, [](auto pro, auto epi, const IgemmArgs& a, hipStream_t s) {
    launch_patch_t<BN, WM, WN, decltype(epi)::value, decltype(pro)::value>(a, s);
  }, kFusionPairs);
}

// Calls f with every runtime bool turned into a std::bool_constant argument, so that f can name
// the kernel instantiation the bools select.
template <class F>
void with_bools(F&& f) { f(); }
template <class F, class... Bs>
void with_bools(F&& f, bool b, Bs... rest) {
  if (b) with_bools([&](auto... c) { f(std::true_type{}, c...); }, rest...);
  else with_bools([&](auto... c) { f(std::false_type{}, c...); }, rest...);
}

// Stores the tile counts of a launch with bco x bkk tiles over N x kcols for the kernels' block
// decode (wg_block) and returns its grid: one block per (split, tile).
inline int wgrad_grid(WgradArgs& a, int bco, int bkk, int kcols) {
  a.nCo = (a.N + bco - 1) / bco;
  a.nKk = (kcols + bkk - 1) / bkk;
  return a.nCo * a.nKk * a.splits;
}

template <int BCO, int BKK, int WM, int WN, bool DEEP = false>
void launch_wgrad(const WgradArgs& a0, hipStream_t s) {
  WgradArgs a = a0;
  const int grid = wgrad_grid(a, BCO, BKK, a.K);
  const size_t lds = (size_t)2 * 64 * (BCO + BKK) * 2;
  with_bools([&](auto pro, auto dpro) {
    hipLaunchKernelGGL((wgrad_tn<BCO, BKK, WM, WN, decltype(pro)::value, decltype(dpro)::value, DEEP>),
                       dim3(grid), dim3(256), lds, s, a);
  }, a.pro_sc != nullptr, a.dY2 != nullptr);
  HIP_CHECK_LAUNCH();
}

template <int BCO, int BKK, int WM, int WN, int SR, int NST, int MF = 16>
void launch_wgrad_pipe(const WgradArgs& a0, hipStream_t s) {
  WgradArgs a = a0;
  const int grid = wgrad_grid(a, BCO, BKK, a.K);
  const size_t lds = (size_t)NST * SR * (BCO + BKK) * 2;
  hipLaunchKernelGGL((wgrad_pipe<BCO, BKK, WM, WN, SR, NST, MF>), dim3(grid), dim3(64 * WM * WN),
                     lds, s, a);
  HIP_CHECK_LAUNCH();
}

// X bytes per 64-row step when every X gather address of wgrad_xp is affine in the step with a
// fixed validity, else 0 (see XLIN).  SIMCLR_WGRAD_XLIN: 0 = the general form everywhere (the
// default), 1 = every admissible shape, 3 = the k x k (MFMA-bound) shapes only.  XLIN makes
// every xp weight gradient 7-12 % faster alone, but the N = 1 step, where the weight gradients
// run hidden on their side stream, was +0.05 ms slower over 10 interleaved rounds
// (profiles/r6_wgrad_pmc.md), so it stays opt-in
static int g_wgrad_xlin = -1;  // -1: not yet read from the environment
int xlin_mode(int mode) {
  if (mode >= 0) g_wgrad_xlin = mode;
  if (g_wgrad_xlin < 0) {
    const char* e = getenv("SIMCLR_WGRAD_XLIN");
    g_wgrad_xlin = e ? atoi(e) : 0;
  }
  return g_wgrad_xlin;
}
inline uint32_t wgrad_x_linear(const WgradArgs& a) {
  const int mode = xlin_mode(-1);
  if (mode == 0 || (mode == 3 && a.K == a.C)) return 0;
  const int ohw = a.OH * a.OW;
  if (a.KW == 1 && a.K == a.C && a.ish == 1 && a.isw == 1 && a.ih0 == 0 && a.iw0 == 0 &&
      a.IH == a.OH && a.IW == a.OW)
    return (uint32_t)(64 * a.C * 2);  // X row m is output row m
  if (ohw > 0 && 64 % ohw == 0)
    return (uint32_t)((size_t)(64 / ohw) * a.IH * a.IW * a.C * 2);  // n advances, (oh, ow) kept
  return 0;
}

template <int BCO, int BKK, int WM, int WN, int MF>
void launch_wgrad_xp(const WgradArgs& a0, hipStream_t s) {
  WgradArgs a = a0;
  const int grid = wgrad_grid(a, BCO, BKK, a.K);
  const size_t lds = (size_t)2 * 64 * (BCO + BKK) * 2;
  a.x_step = wgrad_x_linear(a);
  with_bools([&](auto xlin) {
    hipLaunchKernelGGL((wgrad_xp<BCO, BKK, WM, WN, MF, decltype(xlin)::value>), dim3(grid),
                       dim3(64 * WM * WN), lds, s, a);
  }, a.x_step != 0);
  HIP_CHECK_LAUNCH();
}

template <int BCO, int BKK, int WM, int WN, int NST = 2, int MF = 16>
void launch_wgrad_glds(const WgradArgs& a0, hipStream_t s) {
  WgradArgs a = a0;
  const int grid = wgrad_grid(a, BCO, BKK, a.K);
  const size_t lds = (size_t)NST * 64 * (BCO + BKK) * 2 + (a.pro_sc != nullptr ? 16 * BKK : 0);
  with_bools([&](auto pro) {
    hipLaunchKernelGGL((wgrad_glds<BCO, BKK, WM, WN, decltype(pro)::value, NST, MF>), dim3(grid),
                       dim3(64 * WM * WN), lds, s, a);
  }, a.pro_sc != nullptr);
  HIP_CHECK_LAUNCH();
}

void launch_wgrad_patch(const WgradArgs& a0, hipStream_t s) {
  WgradArgs a = a0;
  const int grid = wgrad_grid(a, 64, 64, a.C);  // N % 64 == 0 and C % 64 == 0 (wgrad_variant_ok)
  const int pp = (256 / a.OW + 2) * (a.OW + 2);
  const size_t lds = (size_t)2 * (256 * 64 + (pp + 7) / 8 * 512) * 2 +
                     (a.pro_sc != nullptr ? (size_t)2 * 2 * 64 * 4 : 0);
  with_bools([&](auto pro, auto ow32) {
    hipLaunchKernelGGL((wgrad_patch<decltype(pro)::value, decltype(ow32)::value ? 32 : 16>),
                       dim3(grid), dim3(576), lds, s, a);
  }, a.pro_sc != nullptr, a.OW == 32);
  HIP_CHECK_LAUNCH();
}

// ---- tile variants: one row per variant; its position is its number (bench/tiles_mi355x.json and
// the tuning keys pin numbers: append, never reorder).  A row is made from the template arguments
// of its launcher, so the table and the instantiation cannot disagree.
struct IgemmVariant {
  IgFam fam;
  int bm, bn, wm, wn, stages;
  void (*launch)(const IgemmArgs&, hipStream_t);
  constexpr int threads() const { return 64 * wm * wn; }
  constexpr bool fuses(int pro, int epi) const {
    return igemm_fusion_allowed(fam, pro, epi, bm * bn, stages);
  }
};
template <int BM, int BN, int WM, int WN>
constexpr IgemmVariant ig_nt() { return {IG_NT, BM, BN, WM, WN, 2, launch_igemm<BM, BN, WM, WN>}; }
template <int BM, int BN, int WM, int WN, int NST = 2>
constexpr IgemmVariant ig_glds() {
  return {IG_GLDS, BM, BN, WM, WN, NST, launch_glds<BM, BN, WM, WN, NST>};
}
template <int BN, int WM, int WN>
constexpr IgemmVariant ig_patch() { return {IG_PATCH, 256, BN, WM, WN, 2, launch_patch<BN, WM, WN>}; }

constexpr IgemmVariant IG_VARIANTS[] = {
    // 0-6: register-staged kernel (igemm_nt): every geometry and fusion.  The wide-N tiles (5, 6
    // and wgrad 4, 5) cover a whole small output dimension in one tile, so the other operand is
    // streamed from HBM once instead of N/BN (K/BKK) times
    ig_nt<128, 128, 2, 2>(), ig_nt<256, 64, 4, 1>(), ig_nt<128, 64, 2, 2>(), ig_nt<64, 128, 2, 2>(),
    ig_nt<64, 64, 2, 2>(), ig_nt<128, 256, 2, 2>(), ig_nt<64, 256, 1, 4>(),
    // 7-11: LDS-DMA kernel (igemm_glds), two LDS stages: C % 64 == 0
    ig_glds<256, 256, 2, 4>(), ig_glds<256, 128, 4, 2>(), ig_glds<256, 64, 4, 1>(),
    ig_glds<128, 128, 2, 2>(), ig_glds<128, 256, 2, 4>(),
    // 12-14: ... with three LDS stages (no prologue)
    ig_glds<256, 128, 4, 2, 3>(), ig_glds<128, 128, 2, 2, 3>(), ig_glds<128, 256, 2, 4, 3>(),
    // 15, 16: 3x3 stride-1 kernel with an LDS-resident input patch
    ig_patch<64, 4, 1>(), ig_patch<128, 4, 2>(),
    // 17: 2-stage LDS-DMA, 256 x 64 tile on 8 waves (memory-bound 1x1)
    ig_glds<256, 64, 8, 1>(),
    // 18, 19: 2-stage LDS-DMA, one wave column (WN = 1): the BN-apply prologue runs on the A
    // fragments in registers (the short-K 1x1 expansion convs, conv3 of a bottleneck)
    ig_glds<128, 256, 4, 1>(), ig_glds<256, 128, 8, 1>(),
    // 20, 21: single-stage LDS-DMA tiles, 2 blocks per CU (short-K 1x1 convs: one block's loads
    // and epilogue under the other's MFMAs instead of a second LDS stage); BN-apply prologue only
    ig_glds<128, 256, 2, 2, 1>(), ig_glds<256, 128, 2, 2, 1>()};
constexpr int kNumIgemm = (int)(sizeof(IG_VARIANTS) / sizeof(IG_VARIANTS[0]));

enum WgFam { WG_TN, WG_TN_DEEP, WG_GLDS, WG_PATCH, WG_PIPE, WG_XP };
struct WgradVariant {
  WgFam fam;
  int bco, bkk;
  int target;  // resident blocks the split-M count aims at: every split costs an fp32 N x K slab
               // written here and re-read by the reduction, so the LDS-DMA variants (1-2 blocks
               // per CU) aim at 256-512 instead of 768
  int rows;    // output rows per iteration (the unit of a split)
  void (*launch)(const WgradArgs&, hipStream_t);
  // LDS-DMA operand loads: C % 64 == 0, an X prologue only on unpadded 1x1 convolutions
  constexpr bool lds_dma() const { return fam == WG_GLDS || fam == WG_PIPE || fam == WG_XP; }
  constexpr bool x_pro() const { return fam != WG_PIPE && fam != WG_XP; }       // BN-apply on X
  constexpr bool dy_pro() const { return fam == WG_TN || fam == WG_TN_DEEP; }   // BN-backward on dY
  // the patch kernel's K tile is all 9 taps of 64 input channels
  constexpr int k_tiles(int C, int K) const { return fam == WG_PATCH ? C / 64 : (K + bkk - 1) / bkk; }
  constexpr int min_iters() const { return fam == WG_PATCH ? 1 : 8; }  // per split
  // iterations over M output rows: the patch kernel runs whole 256-row iterations only
  constexpr int iters(int M) const { return fam == WG_PATCH ? M / rows : (M + rows - 1) / rows; }
};
template <int BCO, int BKK, int WM, int WN, bool DEEP = false>
constexpr WgradVariant wg_tn(int target) {
  return {DEEP ? WG_TN_DEEP : WG_TN, BCO, BKK, target, 64, launch_wgrad<BCO, BKK, WM, WN, DEEP>};
}
template <int BCO, int BKK, int WM, int WN, int NST = 2, int MF = 16>
constexpr WgradVariant wg_glds(int target) {
  return {WG_GLDS, BCO, BKK, target, 64, launch_wgrad_glds<BCO, BKK, WM, WN, NST, MF>};
}
template <int BCO, int BKK, int WM, int WN, int SR, int NST>
constexpr WgradVariant wg_pipe(int target) {
  return {WG_PIPE, BCO, BKK, target, 64, launch_wgrad_pipe<BCO, BKK, WM, WN, SR, NST>};
}
template <int BCO, int BKK, int WM, int WN, int MF>
constexpr WgradVariant wg_xp(int target) {
  return {WG_XP, BCO, BKK, target, 64, launch_wgrad_xp<BCO, BKK, WM, WN, MF>};
}

constexpr WgradVariant WG_VARIANTS[] = {
    // 0-5: register-staged kernel (wgrad_tn): every geometry and prologue
    wg_tn<128, 128, 2, 2>(768), wg_tn<64, 128, 2, 2>(768), wg_tn<128, 64, 2, 2>(768),
    wg_tn<64, 64, 2, 2>(768), wg_tn<64, 256, 2, 2>(768), wg_tn<256, 64, 2, 2>(768),
    // 6-16: LDS-DMA kernel (wgrad_glds): the X-operand BN-apply prologue only.  4-wave tiles with
    // 128x64 / 64x128 per wave: half the LDS fragment bytes per MFMA of a 64x64 wave tile (the
    // 128x128 wgrad was LDS-bound between DMA writes and tr reads); 13-16 with three LDS stages
    wg_glds<128, 128, 2, 2>(512), wg_glds<256, 128, 2, 2>(256), wg_glds<128, 256, 2, 2>(256),
    wg_glds<256, 256, 2, 4>(256), wg_glds<64, 256, 1, 4>(512), wg_glds<128, 128, 2, 2>(256),
    wg_glds<64, 256, 1, 4>(256), wg_glds<128, 64, 2, 2, 3>(512), wg_glds<128, 128, 2, 2, 3>(256),
    wg_glds<64, 128, 2, 2, 3>(512), wg_glds<256, 128, 2, 2, 3>(256),
    // 17: wgrad_patch (3x3 stride-1, all taps from one input patch, 256-row iterations)
    {WG_PATCH, 64, 64, 256, 256, launch_wgrad_patch},
    // 18, 19: wgrad_tn with loads two steps ahead (DEEP): the 64 x 128 / 128 x 64 tiles gain
    // 10-17 % on the 3x3 / 1x1 weight gradients (tools/wgrad_probe.py); the 128 x 128 and
    // 256 x 64 DEEP tiles spill at the 256-VGPR cap of two blocks per CU and lose (not instantiated)
    wg_tn<64, 128, 2, 2, true>(768), wg_tn<128, 64, 2, 2, true>(768),
    // 20-22: wgrad_pipe (32-row steps, 4-5 LDS stages with all but one in flight), no prologues
    wg_pipe<256, 256, 2, 4, 32, 4>(256), wg_pipe<256, 128, 4, 2, 32, 5>(256),
    wg_pipe<128, 256, 2, 4, 32, 5>(256),
    // 23: wgrad_glds 256 x 256 (8 waves) on v_mfma_f32_32x32x16_bf16 (as 9): half the MFMA and
    // ~17 % fewer VALU instructions, 1-4 % faster on the layer3 / layer4 3x3 weight gradients; the
    // other 32x32x16 tiles and the ping-pong kernel were measured and removed (r4 optimisation log)
    wg_glds<256, 256, 2, 4, 2, 32>(256),
    // 24-26: wgrad_xp (fragment reads carried across the barrier, no prologues) on 32x32x16:
    // 256 x 256 / 256 x 128 (8 waves), 128 x 128 (4 waves)
    wg_xp<256, 256, 2, 4, 32>(256), wg_xp<256, 128, 4, 2, 32>(256), wg_xp<128, 128, 2, 2, 32>(512),
    // 27: wgrad_xp 256 x 256 on 4 waves (128 x 128 per wave, one wave per SIMD): per 64-row step the
    // 8-wave tile reads 196 KB of LDS fragments + 64 KB of DMA writes against ~2,060 MFMA clocks per
    // SIMD (LDS at parity with the MFMAs, 128 B/clk); the 128 x 128 wave tile reads 128 KB (LDS at
    // ~75 % of the MFMA time).  The 256 accumulator registers per lane live in AGPRs.  Measured
    // 15-20 % slower than 24 on every shape (one wave per SIMD: its own VALU address work and DMA
    // issue sit between its MFMAs; profiles/r6_wgrad_pmc.md); kept for the record and the sweep.
    wg_xp<256, 256, 2, 2, 32>(256)};
constexpr int kNumWgrad = (int)(sizeof(WG_VARIANTS) / sizeof(WG_VARIANTS[0]));


// -------------------------------------------------- fused 1x1 backward: dgrad + wgrad in one pass
// A bottleneck's conv3 backward at 32x32 (ResNet-50 layer1: Ci = 64, Co = 256, M = 2^20 rows) is
// HBM-bound on its output gradient: the dgrad reads dY (or g and the pre-BN activation when the
// BN3 backward runs in its prologue: 1 GB), and the weight gradient re-reads the same 1 GB on the
// side stream (r2: 171-235 TF/s, 4.7 ms of weight-gradient wall time per step).  This kernel
// reads every operand once: a persistent block walks its m-tiles (64 rows) of one view segment,
// forms the dY tile (BN-backward prologue in registers) and the X tile (BN2-apply + ReLU) in LDS,
// and per tile
//   dX[64 x Ci]  = dY[64 x Co] · W[Co x Ci]     (Wᵀ resident in LDS; dY read non-transposed)
//   dW[Co x Ci] += dYᵀ[Co x 64] · X[64 x Ci]    (both read with ds_read_b64_tr_b16, registers)
// with the dgrad's mode-3 epilogue (ReLU mask of BN2 from the raw a2 tile, Σg / Σg·x̂ partials of
// the BN2 backward).  At the end each block writes its dW slab (summed by the split reduction)
// and one partial-statistics row.  Reference math: /root/reference/model.py Bottleneck conv3 +
// SyncBatchNorm backward.
struct Dual1x1Args {
  const uint16_t* G;     // [M][CO]: dY, or the BN3-backward input g (lazy)
  const uint16_t* A3;    // [M][CO] pre-BN activation for the lazy form, or nullptr
  const float* coef;     // [3][S][CO] lazy BN-backward coefficients
  const uint16_t* X;     // [M][CI] pre-BN a2 (conv3's forward input before BN2 + ReLU)
  const float* xss;      // [2][S][CI] BN2 scale / shift
  const float* xmi;      // [2][S][CI] BN2 mean / invstd
  const uint16_t* Wt;    // [CI][CO] dgrad weight (transformed OHWI, 1x1)
  uint16_t* gm;          // [M][CI] masked input gradient
  float* stats;          // [S * bps][2][CI] partials Σg, Σg·x̂
  float* wpart;          // [S * bps][CO][CI] dW slabs
  int M, S, seg_rows, bps, tiles_per_block;
  uint32_t g_bytes, x_bytes;
  // wide form only: X already holds relu(bn2(a2)) (the forward materialised it), Xraw = a2 for
  // the epilogue's mask / x̂
  const uint16_t* Xraw;
  int x_pre;
  // plain stride-2 downsample form (conv1x1_bwd_dual_s2): X is the [N][xH][xW][Ci] block input,
  // output pixel (n, oh, ow) of the xOH x xOW map reads input pixel (n, 2 oh, 2 ow)
  int xH, xW, xOH, xOW;
};

// PLAIN (a stride-1 downsample conv of the same shape, layer1.0): no BatchNorm between its input
// and the conv — X is taken as stored, the dgrad output is written unmasked and no partials are
// produced; with the lazy prologue its dY is the downsample BN's backward (A·g + B·ad + D).
template <int CO, int CI, bool PLAIN = false>
__global__ __launch_bounds__(256, 1) void conv1x1_bwd_dual(Dual1x1Args p) {
  static_assert(CO == 256 && CI == 64, "tile mapping written for Co = 256, Ci = 64");
  constexpr int BMT = 64;  // rows per m-tile
  extern __shared__ __attribute__((aligned(16))) char smem[];
  uint16_t* Ds = (uint16_t*)smem;             // [2][64][CO]  tr_swz<CO> image of dY
  uint16_t* Xs = Ds + 2 * BMT * CO;           // [2][64][CI]  tr_swz<CI> image of relu(bn2(a2))
  uint16_t* Xr = Xs + 2 * BMT * CI;           // [2][64][CI]  raw a2 (epilogue mask / x̂)
  uint16_t* Ws = Xr + 2 * BMT * CI;           // [CI][CO]     Wᵀ, chunk ^= row & 7
  float* red = (float*)(Ws + CI * CO);        // [4][CI][2]   statistics reduction
  float* Tb = red + 4 * CI * 2;               // [4][CI]      BN2 tables for the epilogue

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int g = lane >> 4, li = lane & 15;
  const int blk = xcd_remap(blockIdx.x, gridDim.x);
  const int seg = blk / p.bps;
  const int mbeg = seg * p.seg_rows + (blk - seg * p.bps) * p.tiles_per_block * BMT;
  const int T = p.tiles_per_block;
  const bool lazy = p.A3 != nullptr;

  const __amdgpu_buffer_rsrc_t rg = buf_rsrc(p.G, p.g_bytes);
  const __amdgpu_buffer_rsrc_t ra = buf_rsrc(lazy ? p.A3 : p.G, p.g_bytes);
  const __amdgpu_buffer_rsrc_t rx = buf_rsrc(p.X, p.x_bytes);

  // W^T resident for the whole block (one 32 KB read per block)
  for (int c = tid; c < CI * CO / 8; c += 256) {
    const int row = c / (CO / 8), ch = c % (CO / 8);
    *(u32x4*)(Ws + row * CO + ((ch ^ (row & 7)) * 8)) = *(const u32x4*)(p.Wt + (size_t)c * 8);
  }

  // loader mapping: dY chunk column fixed per thread (8 output channels), rows tid/32 + 8j;
  // X chunk column fixed (8 input channels), rows tid/8 + 32j
  constexpr int GCH = CO / 8, XCH = CI / 8;
  const int gch = tid % GCH, grow = tid / GCH;  // rows grow + 8j, j < 8
  const int xch = tid % XCH, xrow = tid / XCH;  // rows xrow + 32j, j < 2
  float cA[8], cB[8], cD[8], xsc[8], xsh[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int co = gch * 8 + e, ci = xch * 8 + e;
    cA[e] = lazy ? p.coef[seg * CO + co] : 1.f;
    cB[e] = lazy ? p.coef[(p.S + seg) * CO + co] : 0.f;
    cD[e] = lazy ? p.coef[(2 * p.S + seg) * CO + co] : 0.f;
    xsc[e] = PLAIN ? 1.f : p.xss[seg * CI + ci];
    xsh[e] = PLAIN ? 0.f : p.xss[(p.S + seg) * CI + ci];
  }
  // epilogue tables (BN2 scale, shift, mean, invstd of this segment) in LDS: [4][CI]
  for (int i = tid; i < (PLAIN ? 0 : 4 * CI); i += 256) {
    const int k = i / CI, c = i % CI;
    Tb[i] = (k < 2 ? p.xss : p.xmi)[((k & 1) * p.S + seg) * CI + c];
  }

  // operand loads run two m-tiles ahead (two register sets, the loop unrolled by two so that
  // every set index is static): one tile's 72 KB per block is too little in flight to cover
  // HBM latency at one block per CU
  u32x4 rG[2][8], rA[2][8], rX[2][2];
  auto gload = [&](int t, u32x4 (&G8)[8], u32x4 (&A8)[8], u32x4 (&X2)[2]) {
    const int m0 = mbeg + t * BMT;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const uint32_t off = (uint32_t)(((size_t)(m0 + grow + 8 * j) * CO + gch * 8) * 2);
      G8[j] = __builtin_amdgcn_raw_buffer_load_b128(rg, off, 0, 0);
      if (lazy) A8[j] = __builtin_amdgcn_raw_buffer_load_b128(ra, off, 0, 0);
    }
#pragma unroll
    for (int j = 0; j < 2; ++j)
      X2[j] = __builtin_amdgcn_raw_buffer_load_b128(
          rx, (uint32_t)(((size_t)(m0 + xrow + 32 * j) * CI + xch * 8) * 2), 0, 0);
  };
  auto lstore = [&](int buf, const u32x4 (&G8)[8], const u32x4 (&A8)[8], const u32x4 (&X2)[2]) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int r = grow + 8 * j;
      *(u32x4*)(Ds + buf * BMT * CO + r * CO + tr_swz<CO>(r, gch * 8)) =
          lazy ? bnbwd8(G8[j], A8[j], cA, cB, cD, true) : G8[j];
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int r = xrow + 32 * j;
      *(u32x4*)(Xs + buf * BMT * CI + r * CI + tr_swz<CI>(r, xch * 8)) =
          PLAIN ? X2[j] : affine_relu8(X2[j], xsc, xsh, true, true);
      if (!PLAIN) *(u32x4*)(Xr + buf * BMT * CI + r * CI + xch * 8) = X2[j];
    }
  };

  f32x4 accw[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) accw[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
  float s1[4][4], s2[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) { s1[i][j] = 0.f; s2[i][j] = 0.f; }

  // tile t computes from LDS buffer t & 1; register set (t + 1) & 1 holds tile t + 1 (stored to
  // LDS at the end of iteration t); the loads of tile t + 2 go into set t & 1 at its start
  auto compute = [&](int t) {
    const int cur = t & 1;
    const uint16_t* Db = Ds + cur * BMT * CO;
    // dgrad: D[ci][m] over k = co; wave owns rows m = wid*16 + li
    f32x4 accd[4];
#pragma unroll
    for (int fn = 0; fn < 4; ++fn) accd[fn] = (f32x4){0.f, 0.f, 0.f, 0.f};
    const int mrow = wid * 16 + li;
#pragma unroll
    for (int ks = 0; ks < CO / 32; ++ks) {
      const int lch = ks * 4 + g;
      const bf16x8 bfr = *(const bf16x8*)(Db + mrow * CO + tr_swz<CO>(mrow, lch * 8));
#pragma unroll
      for (int fn = 0; fn < 4; ++fn) {
        const int wr = fn * 16 + li;
        const bf16x8 af = *(const bf16x8*)(Ws + wr * CO + ((lch ^ (wr & 7)) * 8));
        accd[fn] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, bfr, accd[fn], 0, 0, 0);
      }
    }
    // wgrad: accw[fm][fn] += dY^T · X  (wave owns co = wid*64 .. +64)
    wgrad_mma<CO, CI, 4, 1>(Db, Xs + cur * BMT * CI, accw);
    const int m = mbeg + t * BMT + mrow;
    if constexpr (PLAIN) {
#pragma unroll
      for (int fn = 0; fn < 4; ++fn) {
        const int ci = fn * 16 + 4 * g;
        const u32x2 w = {pack2bf(accd[fn][0], accd[fn][1]), pack2bf(accd[fn][2], accd[fn][3])};
        __builtin_nontemporal_store(w, (u32x2*)(p.gm + (size_t)m * CI + ci));
      }
      return;
    }
    // mode-3 epilogue: g = [bn2(a2) > 0] · round(dX), Σg, Σg·x̂
    const uint16_t* xr = Xr + cur * BMT * CI + mrow * CI;
#pragma unroll
    for (int fn = 0; fn < 4; ++fn) {
      const int ci = fn * 16 + 4 * g;
      const u32x2 yv = *(const u32x2*)(xr + ci);
      const float4 tsc = *(const float4*)(Tb + ci), tsh = *(const float4*)(Tb + CI + ci);
      const float4 tmu = *(const float4*)(Tb + 2 * CI + ci);
      const float4 tin = *(const float4*)(Tb + 3 * CI + ci);
      const float y[4] = {lo_bf(yv.x), hi_bf(yv.x), lo_bf(yv.y), hi_bf(yv.y)};
      const float sc4[4] = {tsc.x, tsc.y, tsc.z, tsc.w}, sh4[4] = {tsh.x, tsh.y, tsh.z, tsh.w};
      const float mu4[4] = {tmu.x, tmu.y, tmu.z, tmu.w}, in4[4] = {tin.x, tin.y, tin.z, tin.w};
      float gv[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float a = bf2f(f2bf(accd[fn][r]));
        gv[r] = y[r] * sc4[r] + sh4[r] > 0.f ? a : 0.f;
        s1[fn][r] += gv[r];
        s2[fn][r] += gv[r] * ((y[r] - mu4[r]) * in4[r]);
      }
      const u32x2 w = {pack2bf(gv[0], gv[1]), pack2bf(gv[2], gv[3])};
      __builtin_nontemporal_store(w, (u32x2*)(p.gm + (size_t)m * CI + ci));
    }
  };

  if (T > 0) {
    gload(0, rG[0], rA[0], rX[0]);
    lstore(0, rG[0], rA[0], rX[0]);
  }
  if (T > 1) gload(1, rG[1], rA[1], rX[1]);
  __syncthreads();
  // raw barriers (LDS counter only): __syncthreads() emits vmcnt(0), which would drain the
  // loads of tile t + 2 issued at the top of the iteration and leave one tile in flight
  for (int t = 0; t < T; t += 2) {
    // even tile t: set 1 holds t + 1, set 0 is free
    if (t + 2 < T) gload(t + 2, rG[0], rA[0], rX[0]);
    compute(t);
    if (t + 1 < T) lstore(1, rG[1], rA[1], rX[1]);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    if (t + 1 >= T) break;
    // odd tile t + 1: set 0 holds t + 2, set 1 is free
    if (t + 3 < T) gload(t + 3, rG[1], rA[1], rX[1]);
    compute(t + 1);
    if (t + 2 < T) lstore(0, rG[0], rA[0], rX[0]);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
  }
  __syncthreads();
  // dW slab of this block: [co][ci]
  float* wp = p.wpart + (size_t)blk * CO * CI;
#pragma unroll
  for (int fm = 0; fm < 4; ++fm)
#pragma unroll
    for (int fn = 0; fn < 4; ++fn)
#pragma unroll
      for (int i = 0; i < 4; ++i)
        wp[(size_t)(wid * 64 + fm * 16 + g * 4 + i) * CI + fn * 16 + li] = accw[fm][fn][i];
  if (PLAIN) return;
  // statistics: lanes sharing channels (same g) sum over li, then the 4 waves through LDS
#pragma unroll
  for (int off = 1; off < 16; off <<= 1)
#pragma unroll
    for (int fn = 0; fn < 4; ++fn)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        s1[fn][r] += __shfl_xor(s1[fn][r], off, 64);
        s2[fn][r] += __shfl_xor(s2[fn][r], off, 64);
      }
  if (li == 0) {
#pragma unroll
    for (int fn = 0; fn < 4; ++fn)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int ci = fn * 16 + 4 * g + r;
        red[(wid * CI + ci) * 2 + 0] = s1[fn][r];
        red[(wid * CI + ci) * 2 + 1] = s2[fn][r];
      }
  }
  __syncthreads();
  if (tid < CI) {
    float a = 0.f, b = 0.f;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      a += red[(w * CI + tid) * 2 + 0];
      b += red[(w * CI + tid) * 2 + 1];
    }
    p.stats[((size_t)blk * 2 + 0) * CI + tid] = a;
    p.stats[((size_t)blk * 2 + 1) * CI + tid] = b;
  }
}

// Wide form of the fused 1x1 backward for Co = 512, Ci = 128 (ResNet-50 layer2 conv3, whose
// backward otherwise reads its 2 x 268 MB BN3-backward operands twice: the dgrad on the chain,
// the weight gradient again on the side stream).  Wᵀ [128][512] alone would fill 128 KB of LDS,
// so a block owns one 64-channel slice of Ci (its Wᵀ slice, 64 KB, resident) and the CIT / 64
// slices of a row range are consecutive logical blocks: xcd_remap puts them on one XCD, so the
// second read of each dY tile is an L2 hit.  32-row m-tiles, 8 waves (the 4-wave form of the
// narrow kernel spilled at this width), two register sets and two LDS buffers: two tiles
// (144 KB with the lazy BN3 operand) in flight per CU.  Per tile, wave w:
//   dX[16 rows (w & 1) x 16 ci (w >> 1)] = dY · W-slice  (mode-3 epilogue: BN2 mask, partials)
//   dW[64 co (w) x 64 ci] += dYᵀ · X-slice
// X is either a2 with BN2 + ReLU applied while staging (XPRE = false) or the forward's
// materialised relu(bn2(a2)) (XPRE, a2 read beside it for the epilogue).  The per-channel
// tables live in LDS (registers are the constraint here).
// PLAIN: a 1x1 stride-2 downsample conv (layer2.0: Co 512, Ci 256) — no BatchNorm between its
// input and the conv, so X is read as stored (at the even positions of the block input, XS2),
// the dgrad output (the compact residual of conv1's dgrad) is written unmasked, no partials.
// BMT = 64 with CO = 256 is the 8-wave form of the narrow kernel (Co 256 / Ci 64, one Ci slice):
// two waves per SIMD overlap one wave's VALU / LDS work (the BN prologue, the epilogue) with the
// other's MFMAs, where the 4-wave conv1x1_bwd_dual issues them in order.
template <int CO, int CIT, bool LAZY, bool XPRE, bool PLAIN = false, bool XS2 = false,
          int BMT = 32>
__global__ __launch_bounds__(512, 1) void conv1x1_bwd_dual_w(Dual1x1Args p) {
  constexpr int CI = 64;   // channels of Ci per block
  constexpr int NH = CIT / CI;
  constexpr int NT = 512;
  constexpr int RG = BMT / 16;        // dgrad row groups of 16 rows
  constexpr int CQ = 8 / RG;          // dgrad channel groups
  constexpr int CW = CI / CQ;         // dgrad channels per wave
  constexpr int NF = CW / 16;         // 16-channel fragments per wave
  static_assert((CO == 512 && BMT == 32) || (CO == 256 && BMT == 64), "dual tile mappings");
  static_assert(CIT % CI == 0 && NF >= 1, "dual tile mapping");
  static_assert(!XS2 || PLAIN, "the strided X form is the plain downsample form");
  static_assert(!XPRE || BMT * (CI / 8) == 256, "XPRE: half the threads load the raw operand");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  uint16_t* Ds = (uint16_t*)smem;          // [2][32][CO]  tr_swz<CO> image of dY
  uint16_t* Xs = Ds + 2 * BMT * CO;        // [2][32][CI]  tr_swz<CI> image of relu(bn2(a2)) (slice)
  // Xr rows padded to XRS = CI + 8 elements (144 bytes): the epilogue's 8-byte reads of 16
  // consecutive rows at one column then hit 16 distinct bank pairs (at 128-byte rows they
  // were 8-way conflicts).  Ws chunks are XORed with row & 15: the dgrad's 16-row b128 reads
  // of one chunk column land on 16 distinct chunks (row & 7 left them 2-way)
  constexpr int XRS = CI + 8;
  uint16_t* Xr = Xs + 2 * BMT * CI;        // [2][32][XRS] raw a2 (slice)
  uint16_t* Ws = Xr + 2 * BMT * XRS;       // [CI][CO]     Wᵀ slice, chunk ^= row & 15
  float* red = (float*)(Ws + CI * CO);     // [RG row groups][CI][2]
  float* Tb = red + RG * CI * 2;           // [4][CI]  BN2 scale, shift, mean, invstd (slice)
  float* Cf = Tb + 4 * CI;                 // [3][CO]  BN3-backward A, B, D (LAZY)

  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);  // wave-uniform (scalar) selects
  const int g = lane >> 4, li = lane & 15;
  const int rh = wid % RG, cq = wid / RG;  // dgrad: row group, channel group of the slice
  const int lb = xcd_remap(blockIdx.x, gridDim.x);
  const int half = lb % NH;
  const int blk = lb / NH;
  const int c0 = half * CI;
  const int seg = blk / p.bps;
  const int mbeg = seg * p.seg_rows + (blk - seg * p.bps) * p.tiles_per_block * BMT;
  const int T = p.tiles_per_block;

  const __amdgpu_buffer_rsrc_t rg = buf_rsrc(p.G, p.g_bytes);
  const __amdgpu_buffer_rsrc_t ra = buf_rsrc(LAZY ? p.A3 : p.G, p.g_bytes);
  // XPRE: threads 256.. load the raw a2 chunk the thread 256 below loads the transformed one of
  const __amdgpu_buffer_rsrc_t rx = buf_rsrc((XPRE && wid >= 4) ? p.Xraw : p.X, p.x_bytes);

  for (int c = tid; c < CI * CO / 8; c += NT) {
    const int row = c / (CO / 8), ch = c % (CO / 8);
    *(u32x4*)(Ws + row * CO + ((ch ^ (row & 15)) * 8)) =
        *(const u32x4*)(p.Wt + ((size_t)(c0 + row) * CO + ch * 8));
  }
  for (int i = tid; i < (PLAIN ? 0 : 4 * CI); i += NT) {
    const int k = i / CI, c = i % CI;
    Tb[i] = (k < 2 ? p.xss : p.xmi)[((k & 1) * p.S + seg) * CIT + c0 + c];
  }
  if (LAZY)
    for (int i = tid; i < 3 * CO; i += NT) {
      const int k = i / CO, c = i % CO;
      Cf[i] = p.coef[(k * p.S + seg) * CO + c];
    }
  constexpr int GCH = CO / 8, XCH = CI / 8;
  constexpr int GR = NT / GCH;         // dY rows per loader pass
  constexpr int GJ = BMT / GR;         // passes per tile
  constexpr int XT = BMT * XCH;        // X chunks per tile: 256 or 512 (one per thread)
  static_assert(XT == 256 || XT == 512, "X chunk mapping");
  const int gch = tid % GCH, grow = tid / GCH;
  const int xt = tid % XT, xch = xt % XCH, xrow = xt / XCH;
  const bool xload = XT == 512 || (XPRE && !PLAIN) || wid < 4;
  const bool xown = XT == 512 || wid < 4;  // this thread's chunk goes to Xs (else: raw, XPRE)

  u32x4 rG[2][GJ], rA[2][GJ], rX[2];
  uint32_t xs_n = 0, xs_oh = 0, xs_ow = 0;  // XS2: the lane's output pixel of the next gload
  if (XS2) {
    const uint32_t m = (uint32_t)(mbeg + xrow), ohw = (uint32_t)(p.xOH * p.xOW);
    xs_n = m / ohw;
    const uint32_t rem = m - xs_n * ohw;
    xs_oh = rem / (uint32_t)p.xOW;
    xs_ow = rem - xs_oh * (uint32_t)p.xOW;
  }
  auto gload = [&](int t, u32x4 (&G8)[GJ], u32x4 (&A8)[GJ], u32x4& X1) {
    const int m0 = mbeg + t * BMT;
#pragma unroll
    for (int j = 0; j < GJ; ++j) {
      const uint32_t off = (uint32_t)(((size_t)(m0 + grow + GR * j) * CO + gch * 8) * 2);
      G8[j] = __builtin_amdgcn_raw_buffer_load_b128(rg, off, 0, 0);
      if (LAZY) A8[j] = __builtin_amdgcn_raw_buffer_load_b128(ra, off, 0, 0);
    }
    if (xload) {
      uint32_t xr_ = (uint32_t)(m0 + xrow);  // (the binding bounds every offset by 2^31)
      if constexpr (XS2) {
        // output pixel -> the input pixel at (2 oh, 2 ow); gload runs in tile order, so the
        // lane's (n, oh, ow) advances by one tile (BMT output pixels) per call
        xr_ = (xs_n * (uint32_t)p.xH + 2u * xs_oh) * (uint32_t)p.xW + 2u * xs_ow;
        xs_ow += BMT;
        while (xs_ow >= (uint32_t)p.xOW) { xs_ow -= (uint32_t)p.xOW; ++xs_oh; }
        while (xs_oh >= (uint32_t)p.xOH) { xs_oh -= (uint32_t)p.xOH; ++xs_n; }
      }
      X1 = __builtin_amdgcn_raw_buffer_load_b128(
          rx, (xr_ * (uint32_t)CIT + (uint32_t)(c0 + xch * 8)) * 2u, 0, 0);
    }
  };
  auto lstore = [&](int buf, const u32x4 (&G8)[GJ], const u32x4 (&A8)[GJ], const u32x4& X1) {
#pragma unroll
    for (int j = 0; j < GJ; ++j) {
      const int r = grow + GR * j;
      u32x4 v = G8[j];
      if (LAZY) v = bnbwd8(G8[j], A8[j], Cf + gch * 8, Cf + CO + gch * 8, Cf + 2 * CO + gch * 8,
                           true);
      *(u32x4*)(Ds + buf * BMT * CO + r * CO + tr_swz<CO>(r, gch * 8)) = v;
    }
    if (xown) {
      *(u32x4*)(Xs + buf * BMT * CI + xrow * CI + tr_swz<CI>(xrow, xch * 8)) =
          (XPRE || PLAIN) ? X1 : affine_relu8(X1, Tb + xch * 8, Tb + CI + xch * 8, true, true);
      if (!XPRE && !PLAIN) *(u32x4*)(Xr + buf * BMT * XRS + xrow * XRS + xch * 8) = X1;
    } else if (XPRE && !PLAIN) {
      *(u32x4*)(Xr + buf * BMT * XRS + xrow * XRS + xch * 8) = X1;
    }
  };

  f32x4 accw[CO / 8 / 16][CI / 16];
#pragma unroll
  for (int i = 0; i < CO / 8 / 16; ++i)
#pragma unroll
    for (int j = 0; j < CI / 16; ++j) accw[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
  float s1[NF][4], s2[NF][4];
#pragma unroll
  for (int fn = 0; fn < NF; ++fn)
#pragma unroll
    for (int r = 0; r < 4; ++r) { s1[fn][r] = 0.f; s2[fn][r] = 0.f; }

  auto compute = [&](int t) {
    const int cur = t & 1;
    const uint16_t* Db = Ds + cur * BMT * CO;
    f32x4 accd[NF];
#pragma unroll
    for (int fn = 0; fn < NF; ++fn) accd[fn] = (f32x4){0.f, 0.f, 0.f, 0.f};
    const int mrow = rh * 16 + li;
#pragma unroll 4
    for (int ks = 0; ks < CO / 32; ++ks) {
      const int lch = ks * 4 + g;
      const bf16x8 bfr = *(const bf16x8*)(Db + mrow * CO + tr_swz<CO>(mrow, lch * 8));
#pragma unroll
      for (int fn = 0; fn < NF; ++fn) {
        const int wr = cq * CW + fn * 16 + li;
        const bf16x8 af = *(const bf16x8*)(Ws + wr * CO + ((lch ^ (wr & 15)) * 8));
        accd[fn] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, bfr, accd[fn], 0, 0, 0);
      }
    }
    wgrad_mma<CO, CI, 8, 1, BMT / 32>(Db, Xs + cur * BMT * CI, accw);
    const int m = mbeg + t * BMT + mrow;
#pragma unroll
    for (int fn = 0; fn < NF; ++fn) {
    const int ci = cq * CW + fn * 16 + 4 * g;
    if constexpr (PLAIN) {
      const u32x2 w = {pack2bf(accd[fn][0], accd[fn][1]), pack2bf(accd[fn][2], accd[fn][3])};
      __builtin_nontemporal_store(w, (u32x2*)(p.gm + (size_t)m * CIT + c0 + ci));
    } else {
    const uint16_t* xr = Xr + cur * BMT * XRS + mrow * XRS;
    const u32x2 yv = *(const u32x2*)(xr + ci);
    const float4 tsc = *(const float4*)(Tb + ci), tsh = *(const float4*)(Tb + CI + ci);
    const float4 tmu = *(const float4*)(Tb + 2 * CI + ci);
    const float4 tin = *(const float4*)(Tb + 3 * CI + ci);
    const float y[4] = {lo_bf(yv.x), hi_bf(yv.x), lo_bf(yv.y), hi_bf(yv.y)};
    const float sc4[4] = {tsc.x, tsc.y, tsc.z, tsc.w}, sh4[4] = {tsh.x, tsh.y, tsh.z, tsh.w};
    const float mu4[4] = {tmu.x, tmu.y, tmu.z, tmu.w}, in4[4] = {tin.x, tin.y, tin.z, tin.w};
    float gv[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float a = bf2f(f2bf(accd[fn][r]));
      gv[r] = y[r] * sc4[r] + sh4[r] > 0.f ? a : 0.f;
      s1[fn][r] += gv[r];
      s2[fn][r] += gv[r] * ((y[r] - mu4[r]) * in4[r]);
    }
    const u32x2 w = {pack2bf(gv[0], gv[1]), pack2bf(gv[2], gv[3])};
    __builtin_nontemporal_store(w, (u32x2*)(p.gm + (size_t)m * CIT + c0 + ci));
    }
    }
  };

  __syncthreads();  // tables in LDS
  if (T > 0) {
    gload(0, rG[0], rA[0], rX[0]);
    lstore(0, rG[0], rA[0], rX[0]);
  }
  if (T > 1) gload(1, rG[1], rA[1], rX[1]);
  __syncthreads();
  // raw barriers (LDS counter only), as in conv1x1_bwd_dual: a vmcnt(0) would drain the loads
  // of tile t + 2 issued at the top of the iteration
  for (int t = 0; t < T; t += 2) {
    if (t + 2 < T) gload(t + 2, rG[0], rA[0], rX[0]);
    if constexpr (PLAIN) __builtin_amdgcn_sched_barrier(0);  // (keeps the loads' live ranges)
    compute(t);
    if constexpr (PLAIN) __builtin_amdgcn_sched_barrier(0);
    if (t + 1 < T) lstore(1, rG[1], rA[1], rX[1]);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    if (t + 1 >= T) break;
    if (t + 3 < T) gload(t + 3, rG[1], rA[1], rX[1]);
    if constexpr (PLAIN) __builtin_amdgcn_sched_barrier(0);
    compute(t + 1);
    if constexpr (PLAIN) __builtin_amdgcn_sched_barrier(0);
    if (t + 2 < T) lstore(0, rG[0], rA[0], rX[0]);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
  }
  __syncthreads();
  float* wp = p.wpart + (size_t)blk * CO * CIT;
#pragma unroll
  for (int fm = 0; fm < CO / 8 / 16; ++fm)
#pragma unroll
    for (int fn = 0; fn < CI / 16; ++fn)
#pragma unroll
      for (int i = 0; i < 4; ++i)
        wp[(size_t)(wid * (CO / 8) + fm * 16 + g * 4 + i) * CIT + c0 + fn * 16 + li] =
            accw[fm][fn][i];
  if (PLAIN) return;
#pragma unroll
  for (int off = 1; off < 16; off <<= 1)
#pragma unroll
    for (int fn = 0; fn < NF; ++fn)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        s1[fn][r] += __shfl_xor(s1[fn][r], off, 64);
        s2[fn][r] += __shfl_xor(s2[fn][r], off, 64);
      }
  if (li == 0) {
#pragma unroll
    for (int fn = 0; fn < NF; ++fn)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int ci = cq * CW + fn * 16 + 4 * g + r;
        red[(rh * CI + ci) * 2 + 0] = s1[fn][r];
        red[(rh * CI + ci) * 2 + 1] = s2[fn][r];
      }
  }
  __syncthreads();
  if (tid < CI) {
    float a = 0.f, b = 0.f;
#pragma unroll
    for (int q = 0; q < RG; ++q) {  // fixed order: deterministic
      a += red[(q * CI + tid) * 2 + 0];
      b += red[(q * CI + tid) * 2 + 1];
    }
    p.stats[((size_t)blk * 2 + 0) * CIT + c0 + tid] = a;
    p.stats[((size_t)blk * 2 + 1) * CIT + c0 + tid] = b;
  }
}

}  // namespace

void conv_weight_transform_batch(const WtDesc* d, int n, int total_blocks, hipStream_t s) {
  hipLaunchKernelGGL(weight_transform_batch, dim3(total_blocks), dim3(256), 0, s, d, n);
  HIP_CHECK_LAUNCH();
}

int igemm_num_variants() { return kNumIgemm; }
int igemm_variant_bm(int v) { return IG_VARIANTS[v].bm; }
int igemm_variant_bn(int v) { return IG_VARIANTS[v].bn; }
int igemm_default_variant(int N) { return N <= 64 ? 1 : 0; }
bool igemm_variant_glds(int v) { return v >= 0 && v < kNumIgemm && IG_VARIANTS[v].fam != IG_NT; }
bool igemm_variant_patch(int v) {
  return v >= 0 && v < kNumIgemm && IG_VARIANTS[v].fam == IG_PATCH;
}
bool igemm_glds_ok(const ConvGeom& g, bool pro, bool bn_bwd_pro) {
  if (g.C % 64 != 0) return false;
  // the BN-apply / BN-backward prologues run on the landed tile: only valid without
  // zero-padding taps
  return !(pro || bn_bwd_pro) || (g.KH == 1 && g.KW == 1 && g.ih0 == 0 && g.iw0 == 0);
}
static bool direct_out(const ConvGeom& g) {
  return g.osh == 1 && g.osw == 1 && g.ooh == 0 && g.oow == 0 && g.OHp == g.OH && g.OWp == g.OW;
}
bool igemm_patch_ok(const ConvGeom& g) {
  return g.KH == 3 && g.KW == 3 && g.ish == 1 && g.isw == 1 && g.dh == 1 && g.dw == 1 &&
         g.ih0 == -1 && g.iw0 == -1 && g.OH == g.IH && g.OW == g.IW &&
         (g.OW == 16 || g.OW == 32) && (g.C == 64 || g.C == 128) && direct_out(g);
}
// LDS-DMA tile with the doubled A staging of PRO 2 / 3 and `words` fp32 table words per channel
static bool glds_doubled_fits(const IgemmVariant& r, const ConvGeom& g, int words) {
  const size_t lds = igemm_glds_pro_offset(r.bm, r.bn, r.threads(), g.C > 64 ? 2 : 1, 2) +
                     (size_t)4 * words * g.C;
  return lds <= 160 * 1024;
}
// block-output prologue (PRO 3): 2-stage LDS-DMA tiles whose doubled A staging fits the LDS,
// on 1x1 / stride-1 / unpadded / direct-output convolutions (A row m = output row m)
bool igemm_dual_ok(int v, const ConvGeom& g) {
  if (v < 0 || v >= kNumIgemm) return false;
  const IgemmVariant& r = IG_VARIANTS[v];
  if (!r.fuses(3, 0) || !igemm_glds_ok(g, true, false)) return false;
  if (!(direct_out(g) && g.ish == 1 && g.isw == 1 && g.OH == g.IH && g.OW == g.IW)) return false;
  if ((g.Nb * g.OH * g.OW) % r.bm) return false;  // whole tiles: the kernel counts its stores
  return glds_doubled_fits(r, g, 4);
}

bool igemm_variant_ok(int v, const ConvGeom& g, bool pro, bool bn_bwd_pro, int epi_mode) {
  if (v < 0 || v >= kNumIgemm) return false;
  const IgemmVariant& r = IG_VARIANTS[v];
  // the epilogue matters where it depends on the tile: the LDS-DMA kernel's BN-backward prologue
  // with mode 4.  (The holes that do not depend on the tile are fusion rules of the bindings.)
  const bool bwd4 = bn_bwd_pro && (epi_mode & 255) == 4 && r.fam == IG_GLDS;
  if (!r.fuses(igemm_pro_code(pro, bn_bwd_pro, false), bwd4 ? 4 : 0)) return false;
  switch (r.fam) {
    case IG_NT: return true;  // every geometry
    case IG_PATCH: {
      if (!igemm_patch_ok(g)) return false;
      if (!bn_bwd_pro) return true;
      // BN-backward prologue: its second operand must fit the per-thread register stage
      // (kPatchBnbChunks chunks of the patch per thread)
      const int TR = 256 / g.OW, PP = (TR + 2) * (g.OW + 2), NT = r.threads();
      return (PP * (g.C / 8) + NT - 1) / NT <= kPatchBnbChunks;
    }
    case IG_GLDS:  // PRO 2 stages dY and x: doubled A staging + a 3 x C table must fit
      return (!bn_bwd_pro || glds_doubled_fits(r, g, 3)) && igemm_glds_ok(g, pro, bn_bwd_pro);
  }
  return false;
}
int igemm_block_m(int N) { return igemm_variant_bm(igemm_default_variant(N)); }

void conv_igemm_nt(const ConvGeom& g, const uint16_t* A, size_t a_elems, const uint16_t* B,
                   uint16_t* out, const float* bias, float* stats, const ConvFusion& f,
                   int variant, hipStream_t s) {
  IgemmArgs a{};
  a.A = A; a.B = B; a.out = out; a.bias = bias; a.stats = stats;
  a.M = g.Nb * g.OH * g.OW; a.N = g.N; a.K = g.KH * g.KW * g.C;
  a.IH = g.IH; a.IW = g.IW; a.C = g.C;
  a.OH = g.OH; a.OW = g.OW; a.KW = g.KW;
  a.ish = g.ish; a.isw = g.isw; a.dh = g.dh; a.dw = g.dw; a.ih0 = g.ih0; a.iw0 = g.iw0;
  a.OHp = g.OHp; a.OWp = g.OWp; a.osh = g.osh; a.osw = g.osw; a.ooh = g.ooh; a.oow = g.oow;
  a.ldo = g.ldo;
  a.direct_out = direct_out(g) ? 1 : 0;
  a.a_bytes = (uint32_t)(a_elems * 2);
  a.b_bytes = (uint32_t)((size_t)a.N * a.K * 2);
  a.pro_sc = f.pro_sc; a.pro_sh = f.pro_sh; a.pro_seg_rows = f.pro_seg_rows > 0 ? f.pro_seg_rows : a.M;
  a.pro_relu = f.pro_relu;
  a.pro_d = f.pro_d; a.A2 = f.A2;
  a.pro_rsc = f.pro_rsc; a.pro_rsh = f.pro_rsh; a.pro_out = f.pro_out; a.pro_mask = f.pro_mask;
  a.epi_mode = f.epi_mode; a.epi_a_sub = f.epi_a_sub; a.epi_a = f.epi_a; a.epi_b = f.epi_b; a.epi_c = f.epi_c;
  a.epi_mask = f.epi_mask;
  a.epi_c2 = f.epi_c2; a.epi_mi2 = f.epi_mi2; a.stats2 = f.stats2;
  a.epi_ss = f.epi_ss; a.epi_mi = f.epi_mi; a.epi_S = f.epi_S > 0 ? f.epi_S : 1;
  a.seg_rows = f.seg_rows; a.stats_seg_blocks = f.stats_seg_blocks; a.stats_base = f.stats_base;
  if (variant < 0 || variant >= igemm_num_variants()) variant = igemm_default_variant(g.N);
  const bool dual = a.pro_out != nullptr && a.pro_d == nullptr;  // (with pro_d: materialised
                                                                 //  BN-backward operand, patch)
  if (dual ? !igemm_dual_ok(variant, g)
           : !igemm_variant_ok(variant, g, a.pro_sc != nullptr, a.pro_d != nullptr, a.epi_mode)) {
    fprintf(stderr, "igemm: variant %d: unsupported geometry / fusion\n", variant);
    abort();  // the bindings reject this; never silently change BM (stats layout)
  }
  IG_VARIANTS[variant].launch(a, s);
}


int wgrad_num_variants() { return kNumWgrad; }
int wgrad_xlin(int mode) { return xlin_mode(mode); }
int wgrad_default_variant(int N) { return N <= 64 ? 1 : 0; }
bool wgrad_variant_glds(int v) { return v >= 0 && v < kNumWgrad && WG_VARIANTS[v].lds_dma(); }
int wgrad_variant_area(int v) { return WG_VARIANTS[v].bco * WG_VARIANTS[v].bkk; }
bool wgrad_variant_ok(int v, const ConvGeom& g, bool pro, bool dy_pro) {
  if (v < 0 || v >= kNumWgrad) return false;
  const WgradVariant& r = WG_VARIANTS[v];
  if ((pro && !r.x_pro()) || (dy_pro && !r.dy_pro())) return false;
  if (r.fam == WG_PATCH) return g.N % 64 == 0 && igemm_patch_ok(g);
  return !r.lds_dma() || igemm_glds_ok(g, pro, false);
}

int wgrad_tiles(const ConvGeom& g, int variant) {
  if (variant < 0 || variant >= kNumWgrad) variant = wgrad_default_variant(g.N);
  const WgradVariant& r = WG_VARIANTS[variant];
  return ((g.N + r.bco - 1) / r.bco) * r.k_tiles(g.C, g.KH * g.KW * g.C);
}

int wgrad_splits(const ConvGeom& g, int variant) {
  if (variant < 0 || variant >= kNumWgrad) variant = wgrad_default_variant(g.N);
  const WgradVariant& r = WG_VARIANTS[variant];
  const int tiles = wgrad_tiles(g, variant);
  const int iters = r.iters(g.Nb * g.OH * g.OW);
  // The weight gradients run on their own stream beside the dgrad / BatchNorm chain, so they
  // need not fill the chip alone, and every split costs an fp32 N x K slab written here and
  // re-read by the split reduction: the step is fastest at ~60-80 % of the targets tuned for a
  // weight gradient running alone (A/B of SIMCLR_WGRAD_TARGET_PCT, ResNet-50 step: 25 % 23.68,
  // 35 % 22.98, 50 % 22.83, 70 % 22.74, 100 % 23.24, 200 % 23.16 ms)
  static const int pct = [] {
    const char* e = getenv("SIMCLR_WGRAD_TARGET_PCT");
    const int v = e ? atoi(e) : 80;  // end of round 3: 80 beat 60 in 5 of 5 A/B rounds
    return v > 0 ? v : 100;
  }();
  const int target = std::max(1, r.target * pct / 100);
  const int splits = (target + tiles - 1) / tiles;
  return std::max(1, std::min(splits, iters / r.min_iters()));
}

// ---- split reduction over [splits][4 * n4] fp32 slabs: one column-parallel kernel where it
// applies, else groups of 16 slabs pre-summed in place, then the float4 sum into the output
struct SlabsLeft { int count, stride; };  // slabs still to be summed, `stride` slabs apart
static SlabsLeft reduce_slabs_l1(float* partial, int splits, size_t n4, hipStream_t s) {
  constexpr int GROUP = 16;
  if (splits <= 2 * GROUP) return {splits, 1};
  const int G = (splits + GROUP - 1) / GROUP;
  const int bx = (int)std::min<size_t>((n4 + 255) / 256, 1024);
  hipLaunchKernelGGL(wgrad_reduce_l1, dim3(bx, G), dim3(256), 0, s, (float4*)partial, splits,
                     GROUP, n4);
  HIP_CHECK_LAUNCH();
  return {G, GROUP};
}
// vec4: the slab size is a multiple of 4 floats (else only the final sum runs, on the whole float4s)
static void reduce_slabs(float* partial, int splits, float* out, size_t n4, float beta, bool vec4,
                         hipStream_t s) {
  if (vec4 && reduce_cols_ok(n4, splits)) {
    hipLaunchKernelGGL(wgrad_reduce_cols, dim3((unsigned)((n4 + RC_COLS - 1) / RC_COLS)),
                       dim3(256), 0, s, (const float4*)partial, (float4*)out, splits, n4, beta);
    HIP_CHECK_LAUNCH();
    return;
  }
  const SlabsLeft left = vec4 ? reduce_slabs_l1(partial, splits, n4, s) : SlabsLeft{splits, 1};
  const int blocks = (int)std::min<size_t>((n4 + 255) / 256, 8192);
  hipLaunchKernelGGL(wgrad_reduce_vec4, dim3(blocks), dim3(256), 0, s, (const float4*)partial,
                     (float4*)out, left.count, left.stride, n4, beta);
  HIP_CHECK_LAUNCH();
}

void conv_wgrad(const ConvGeom& g, const uint16_t* dY, const uint16_t* X, size_t x_elems,
                float* partial, int splits, float* out, int Creal, float beta,
                const ConvFusion& f, int variant, hipStream_t s) {
  WgradArgs a{};
  a.dY = dY; a.X = X; a.partial = partial;
  a.M = g.Nb * g.OH * g.OW; a.N = g.N; a.K = g.KH * g.KW * g.C;
  a.IH = g.IH; a.IW = g.IW; a.C = g.C;
  a.OH = g.OH; a.OW = g.OW; a.KW = g.KW;
  a.ish = g.ish; a.isw = g.isw; a.dh = g.dh; a.dw = g.dw; a.ih0 = g.ih0; a.iw0 = g.iw0;
  a.dy_bytes = (uint32_t)((size_t)a.M * a.N * 2);
  a.x_bytes = (uint32_t)(x_elems * 2);
  if (variant < 0 || variant >= kNumWgrad) variant = wgrad_default_variant(g.N);
  const WgradVariant& r = WG_VARIANTS[variant];
  const int iters = r.iters(a.M);
  a.splits = splits;
  a.iters_per_split = (iters + splits - 1) / splits;
  a.pro_sc = f.pro_sc; a.pro_sh = f.pro_sh;
  a.pro_seg_rows = f.pro_seg_rows > 0 ? f.pro_seg_rows : a.M;
  a.pro_relu = f.pro_relu; a.pro_S = f.pro_S > 0 ? f.pro_S : 1;
  a.dY2 = f.dY2; a.dp_coef = f.dp_coef; a.dp_seg_rows = f.dp_seg_rows > 0 ? f.dp_seg_rows : a.M;
  a.dp_S = f.dp_S > 0 ? f.dp_S : 1;
  a.slab_stride = (size_t)a.N * a.K;
  // attribution experiment (bench.py / tools only; refused by the training entry points):
  // SIMCLR_EXPERIMENT_WGRAD_SLABS=noreduce skips the split reductions, =alias also makes every
  // split write slab 0 (the weight gradients are garbage; what remains is the step without the
  // split-slab traffic)
  static const int slab_exp = [] {
    const char* e = getenv("SIMCLR_EXPERIMENT_WGRAD_SLABS");
    if (!e) return 0;
    if (!strcmp(e, "noreduce")) return 1;
    if (!strcmp(e, "alias")) return 2;
    return 0;
  }();
  if (slab_exp == 2) a.slab_stride = 0;
  if (!wgrad_variant_ok(variant, g, a.pro_sc != nullptr, a.dY2 != nullptr)) {
    fprintf(stderr, "wgrad: variant %d: unsupported geometry / prologue\n", variant);
    abort();  // the bindings reject this
  }
  r.launch(a, s);
  const int K = a.K;
  // one split writing its slab straight into the output (the caller passed partial == out): the
  // slab IS the [N][K] fp32 gradient, no reduction launch
  if (splits == 1 && partial == out && Creal == g.C && beta == 0.f) return;
  if (slab_exp != 0) return;
  const size_t n4 = (size_t)a.N * K / 4;
  const bool vec4 = (a.N * K) % 4 == 0;
  if (Creal == g.C) {
    reduce_slabs(partial, splits, out, n4, beta, vec4, s);
    return;
  }
  // channel-padded input (the stem: 3 image channels gathered as 8)
  const SlabsLeft left = vec4 ? reduce_slabs_l1(partial, splits, n4, s) : SlabsLeft{splits, 1};
  const size_t total = (size_t)a.N * (K / g.C) * Creal;
  const int cb = (int)std::min<size_t>((total + 255) / 256, 4096);
  if (left.count > 1 && vec4) {
    // the slabs are summed with float4 loads into slab 0 in place (each element owned by one
    // thread), then slab 0 is compacted to the Creal channels — the scalar strided reduction
    // over many slabs was 46 µs at the very end of the backward
    const int blocks = (int)std::min<size_t>((n4 + 255) / 256, 8192);
    hipLaunchKernelGGL(wgrad_reduce_vec4_inplace, dim3(blocks), dim3(256), 0, s,
                       (float4*)partial, left.count, left.stride, n4);
    HIP_CHECK_LAUNCH();
    hipLaunchKernelGGL(wgrad_reduce, dim3(cb), dim3(256), 0, s, partial, out, 1, 1, a.N, K, g.C,
                       Creal, beta);
  } else {
    hipLaunchKernelGGL(wgrad_reduce, dim3(cb), dim3(256), 0, s, partial, out, left.count,
                       left.stride, a.N, K, g.C, Creal, beta);
  }
  HIP_CHECK_LAUNCH();
}

void conv_weight_transform(const uint16_t* W, uint16_t* Wt, int Co, int KH, int KW, int Ci,
                           int KHs, int KWs, int kh0, int sh, int kw0, int sw, hipStream_t s) {
  const size_t total = (size_t)Ci * KHs * KWs * Co;
  int blocks = (int)((total + 255) / 256);
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(weight_transform, dim3(blocks), dim3(256), 0, s, W, Wt, Co, KH, KW, Ci, KHs,
                     KWs, kh0, sh, kw0, sw);
  HIP_CHECK_LAUNCH();
}

size_t conv1x1_bwd_dual_lds() {
  return (size_t)2 * 64 * 256 * 2 + 2 * (size_t)2 * 64 * 64 * 2 + (size_t)64 * 256 * 2 +
         (size_t)4 * 64 * 2 * 4 + (size_t)4 * 64 * 4;
}

size_t conv1x1_bwd_dual_w_lds(int CO, int BMT = 32) {
  return (size_t)2 * BMT * CO * 2 + (size_t)2 * BMT * (64 + 72) * 2 + (size_t)64 * CO * 2 +
         (size_t)(BMT / 16) * 64 * 2 * 4 + (size_t)4 * 64 * 4 + (size_t)3 * CO * 4;
}

void conv1x1_bwd_dual(const uint16_t* G, const uint16_t* A3, const float* coef, const uint16_t* X,
                      const float* xss, const float* xmi, const uint16_t* Wt, uint16_t* gm,
                      float* stats, float* wpart, int M, int CO, int CI, int S, int bps,
                      hipStream_t s, const uint16_t* Xraw, bool dual8) {
  Dual1x1Args a{};
  a.G = G; a.A3 = A3; a.coef = coef; a.X = X; a.xss = xss; a.xmi = xmi; a.Wt = Wt; a.gm = gm;
  a.stats = stats; a.wpart = wpart;
  a.M = M; a.S = S; a.seg_rows = M / S; a.bps = bps;
  a.tiles_per_block = a.seg_rows / 64 / bps;
  a.g_bytes = (uint32_t)((size_t)M * CO * 2);
  a.x_bytes = (uint32_t)((size_t)M * CI * 2);
  a.Xraw = Xraw;
  a.x_pre = Xraw != nullptr;
  const size_t lds = conv1x1_bwd_dual_lds();
  if (CO == 512 && CI == 128) {
    a.tiles_per_block = a.seg_rows / 32 / bps;  // 32-row m-tiles
    const dim3 grid(S * bps * 2), blk(512);
    const size_t wl = conv1x1_bwd_dual_w_lds(512);
    if (A3 != nullptr && Xraw != nullptr)
      hipLaunchKernelGGL((conv1x1_bwd_dual_w<512, 128, true, true>), grid, blk, wl, s, a);
    else if (A3 != nullptr)
      hipLaunchKernelGGL((conv1x1_bwd_dual_w<512, 128, true, false>), grid, blk, wl, s, a);
    else if (Xraw != nullptr)
      hipLaunchKernelGGL((conv1x1_bwd_dual_w<512, 128, false, true>), grid, blk, wl, s, a);
    else
      hipLaunchKernelGGL((conv1x1_bwd_dual_w<512, 128, false, false>), grid, blk, wl, s, a);
  } else if (CO == 256 && CI == 64 && Xraw == nullptr && dual8) {
    // 8-wave form (64-row tiles)
    const dim3 grid(S * bps), blk(512);
    const size_t wl = conv1x1_bwd_dual_w_lds(256, 64);
    if (xss == nullptr && A3 != nullptr)
      hipLaunchKernelGGL((conv1x1_bwd_dual_w<256, 64, true, false, true, false, 64>), grid, blk,
                         wl, s, a);
    else if (xss == nullptr)
      hipLaunchKernelGGL((conv1x1_bwd_dual_w<256, 64, false, false, true, false, 64>), grid, blk,
                         wl, s, a);
    else if (A3 != nullptr)
      hipLaunchKernelGGL((conv1x1_bwd_dual_w<256, 64, true, false, false, false, 64>), grid, blk,
                         wl, s, a);
    else
      hipLaunchKernelGGL((conv1x1_bwd_dual_w<256, 64, false, false, false, false, 64>), grid,
                         blk, wl, s, a);
  } else if (CO == 256 && CI == 64 && xss == nullptr) {
    hipLaunchKernelGGL((conv1x1_bwd_dual<256, 64, true>), dim3(S * bps), dim3(256), lds, s, a);
  } else if (CO == 256 && CI == 64 && Xraw == nullptr) {
    hipLaunchKernelGGL((conv1x1_bwd_dual<256, 64>), dim3(S * bps), dim3(256), lds, s, a);
  } else {
    fprintf(stderr, "conv1x1_bwd_dual: unsupported Co=%d Ci=%d\n", CO, CI);
    abort();  // the bindings reject this
  }
  HIP_CHECK_LAUNCH();
}

// layer2.0's 1x1 stride-2 downsample backward (Co 512, Ci 256): compact input gradient and
// weight-gradient slabs from one pass over g and ad (lazy BN backward when A3 is given)
void conv1x1_bwd_dual_s2(const uint16_t* G, const uint16_t* A3, const float* coef,
                         const uint16_t* X, const uint16_t* Wt, uint16_t* gm, float* wpart,
                         int Mo, int CO, int CI, int S, int bps, int H, int W, int OH, int OW,
                         hipStream_t s) {
  Dual1x1Args a{};
  a.G = G; a.A3 = A3; a.coef = coef; a.X = X; a.Wt = Wt; a.gm = gm; a.wpart = wpart;
  a.M = Mo; a.S = S; a.seg_rows = Mo / S; a.bps = bps;
  a.tiles_per_block = a.seg_rows / 32 / bps;
  a.g_bytes = (uint32_t)((size_t)Mo * CO * 2);
  a.x_bytes = (uint32_t)((size_t)(Mo / (OH * OW)) * H * W * CI * 2);
  a.xH = H; a.xW = W; a.xOH = OH; a.xOW = OW;
  if (CO != 512 || CI != 256) {
    fprintf(stderr, "conv1x1_bwd_dual_s2: unsupported Co=%d Ci=%d\n", CO, CI);
    abort();  // the bindings reject this
  }
  const dim3 grid(S * bps * (CI / 64)), blk(512);
  const size_t wl = conv1x1_bwd_dual_w_lds(512);
  // (the lazy-prologue instantiation of this form spilled 58 VGPRs at 8 waves: the caller
  // materialises dY, the binding rejects A3)
  hipLaunchKernelGGL((conv1x1_bwd_dual_w<512, 256, false, false, true, true>), grid, blk, wl, s,
                     a);
  HIP_CHECK_LAUNCH();
}

// out[n] (+)= Σ_s slabs (the split reduction of conv_wgrad, for producers that write
// [splits][N*K] fp32 slabs themselves)
void wgrad_reduce_slabs(float* partial, int splits, float* out, size_t n, float beta,
                        hipStream_t s) {
  reduce_slabs(partial, splits, out, n / 4, beta, true, s);
}

