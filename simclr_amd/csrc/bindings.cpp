// torch.ops.simclr_amd.* registrations for the gfx950 kernels.  Every op launches on the current
// HIP stream (so they compose with hipGraph capture and side-stream overlap) and validates the
// shapes / dtypes / devices the kernels assume before any launch (a bad shape must never reach a
// hand-written kernel: an out-of-bounds access can take the whole node down).
#include <ATen/core/Tensor.h>
#include <ATen/ops/empty.h>
#include <ATen/ops/zeros.h>
#include <ATen/hip/HIPContext.h>
#include <c10/util/Exception.h>
#include <torch/library.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "kernels.h"

using at::Tensor;

namespace {

hipStream_t cur_stream() { return at::hip::getCurrentHIPStream().stream(); }

void check_dev(const Tensor& t, at::ScalarType dt, const char* name) {
  TORCH_CHECK(t.is_cuda(), name, ": expected a GPU tensor");
  TORCH_CHECK(t.scalar_type() == dt, name, ": expected dtype ", dt, " got ", t.scalar_type());
  TORCH_CHECK(t.is_contiguous(), name, ": expected a contiguous tensor");
}

const uint16_t* bf(const Tensor& t, const char* n) {
  check_dev(t, at::kBFloat16, n);
  return reinterpret_cast<const uint16_t*>(t.data_ptr());
}
uint16_t* bfw(const Tensor& t, const char* n) {
  check_dev(t, at::kBFloat16, n);
  return reinterpret_cast<uint16_t*>(t.data_ptr());
}
const float* f32(const Tensor& t, const char* n) {
  check_dev(t, at::kFloat, n);
  return t.data_ptr<float>();
}
float* f32w(const Tensor& t, const char* n) {
  check_dev(t, at::kFloat, n);
  return t.data_ptr<float>();
}
const float* optf32(const c10::optional<Tensor>& t, const char* n) {
  return (t.has_value() && t->defined()) ? f32(*t, n) : nullptr;
}
float* optf32w(const c10::optional<Tensor>& t, const char* n) {
  return (t.has_value() && t->defined()) ? f32w(*t, n) : nullptr;
}
const uint16_t* optbf(const c10::optional<Tensor>& t, const char* n) {
  return (t.has_value() && t->defined()) ? bf(*t, n) : nullptr;
}
uint16_t* optbfw(const c10::optional<Tensor>& t, const char* n) {
  return (t.has_value() && t->defined()) ? bfw(*t, n) : nullptr;
}
const int* i32(const Tensor& t, const char* n) {
  check_dev(t, at::kInt, n);
  return t.data_ptr<int>();
}

ConvGeom geom_from(const std::vector<int64_t>& v) {
  TORCH_CHECK(v.size() == 22, "conv geometry must have 22 entries");
  ConvGeom g;
  int* p = &g.Nb;
  for (int i = 0; i < 22; ++i) p[i] = (int)v[i];
  TORCH_CHECK(g.C % 8 == 0, "conv: gathered channels must be a multiple of 8, got ", g.C);
  TORCH_CHECK(g.N > 0 && g.Nb > 0 && g.OH > 0 && g.OW > 0, "conv: empty problem");
  return g;
}

// ------------------------------------------------------------------------------- conv
ConvFusion fusion_from(const c10::optional<Tensor>& pro_sc, const c10::optional<Tensor>& pro_sh,
                       int64_t pro_seg_rows, bool pro_relu, int64_t pro_S, int64_t epi_mode,
                       const c10::optional<Tensor>& epi_a, const c10::optional<Tensor>& epi_b,
                       int64_t C, int64_t out_numel) {
  ConvFusion f;
  f.pro_sc = optf32(pro_sc, "pro_sc");
  f.pro_sh = optf32(pro_sh, "pro_sh");
  TORCH_CHECK((f.pro_sc == nullptr) == (f.pro_sh == nullptr), "prologue needs scale and shift");
  if (f.pro_sc) {
    TORCH_CHECK(pro_sc->numel() >= pro_S * C && pro_sh->numel() >= pro_S * C,
                "prologue scale/shift must be [S][C]");
  }
  f.pro_seg_rows = (int)pro_seg_rows;
  f.pro_relu = pro_relu ? 1 : 0;
  f.pro_S = (int)pro_S;
  f.epi_mode = (int)epi_mode;
  f.epi_a = optbf(epi_a, "epi_a");
  f.epi_b = optbf(epi_b, "epi_b");
  TORCH_CHECK(epi_mode >= 0 && epi_mode <= 4, "epi_mode");
  if (epi_mode == 1 || epi_mode == 2 || epi_mode == 4)
    TORCH_CHECK(f.epi_a && epi_a->numel() >= out_numel, "epilogue operand a");
  if (epi_mode == 2 || epi_mode == 3)
    TORCH_CHECK(f.epi_b && epi_b->numel() >= out_numel, "epilogue operand b");
  return f;
}

unsigned* tickets_for(const Tensor& like, int64_t n, int64_t slot);


void igemm(const Tensor& A, const Tensor& B, const Tensor& out, const c10::optional<Tensor>& bias,
           const c10::optional<Tensor>& stats, std::vector<int64_t> gv,
           const c10::optional<Tensor>& pro_sc, const c10::optional<Tensor>& pro_sh,
           int64_t pro_seg_rows, bool pro_relu, int64_t epi_mode,
           const c10::optional<Tensor>& epi_a, const c10::optional<Tensor>& epi_b,
           int64_t variant, const c10::optional<Tensor>& epi_ss,
           const c10::optional<Tensor>& epi_mi, int64_t seg_rows, int64_t stats_seg_blocks,
           int64_t stats_base, const c10::optional<Tensor>& epi_c,
           const c10::optional<Tensor>& epi_mask, const c10::optional<Tensor>& epi_c2,
           const c10::optional<Tensor>& epi_mi2, const c10::optional<Tensor>& stats2,
           const c10::optional<Tensor>& pro_d, const c10::optional<Tensor>& A2,
           const c10::optional<Tensor>& pro_rss, const c10::optional<Tensor>& pro_out,
           const c10::optional<Tensor>& pro_mask) {
  const ConvGeom g = geom_from(gv);
  // bit 8 of epi_mode: epi_a is the stride-2 subsampled residual (conv.hip epi_load_batch)
  const bool epi_sub = (epi_mode & 256) != 0;
  epi_mode &= 255;
  TORCH_CHECK(A.numel() == (int64_t)g.Nb * g.IH * g.IW * g.C, "igemm: A numel mismatch");
  TORCH_CHECK(A.numel() * 2 < (int64_t)1 << 31, "igemm: A larger than 2 GiB");
  const int64_t K = (int64_t)g.KH * g.KW * g.C;
  TORCH_CHECK(B.numel() == (int64_t)g.N * K, "igemm: B numel mismatch");
  TORCH_CHECK(g.ldo % 8 == 0 && g.N % 8 == 0, "igemm: N/ldo must be multiples of 8");
  TORCH_CHECK(out.numel() >= (int64_t)g.Nb * g.OHp * g.OWp * g.ldo, "igemm: out too small");
  TORCH_CHECK(out.numel() * 2 < ((int64_t)1 << 31) * 2, "igemm: out too large");
  if (variant < 0 || variant >= igemm_num_variants()) variant = igemm_default_variant(g.N);
  const int64_t M = (int64_t)g.Nb * g.OH * g.OW;
  const int bm = igemm_variant_bm((int)variant);
  const bool has_pd = pro_d.has_value() && pro_d->defined();
  // pro_out: the block-output prologue's output (dual) — or, with the BN-backward prologue on a
  // patch variant, the materialised prologue result (the weight gradient's dY)
  const bool dual = pro_out.has_value() && pro_out->defined() && !has_pd;
  if (dual) {
    TORCH_CHECK(igemm_dual_ok((int)variant, g),
                "igemm: block-output prologue needs a 2-stage LDS-DMA variant (igemm_dual_ok) on "
                "a 1x1 / stride-1 / unpadded convolution");
  } else {
    TORCH_CHECK(igemm_variant_ok((int)variant, g, pro_sc.has_value() && pro_sc->defined(), has_pd,
                                 (int)epi_mode),
                "igemm: variant ", variant, " is not admissible here: an LDS-DMA variant needs "
                "C % 64 == 0, its prologues (BN-apply, BN-backward) only on unpadded 1x1 "
                "convolutions (2-stage tiles whose staging fits) and, for the BN-backward prologue "
                "with the mode-4 epilogue, a tile of at most 256 x 128; a patch variant needs its "
                "3x3 stride-1 geometry");
  }
  if (bias.has_value() && bias->defined()) TORCH_CHECK(bias->numel() == g.N, "igemm: bias size");
  const bool has_stats = stats.has_value() && stats->defined();
  if (has_stats && stats_seg_blocks == 0)
    TORCH_CHECK(stats->numel() >= ((M + bm - 1) / bm) * 2 * g.N, "igemm: stats buffer too small");
  const bool direct = g.osh == 1 && g.osw == 1 && g.ooh == 0 && g.oow == 0 && g.OHp == g.OH &&
                      g.OWp == g.OW;
  const int64_t sub_numel = (int64_t)g.Nb * ((g.OH + 1) / 2) * ((g.OW + 1) / 2) * g.ldo;
  if (epi_sub) {
    TORCH_CHECK(epi_mode == 1 || epi_mode == 2 || epi_mode == 4,
                "igemm: a subsampled residual needs epilogue mode 1, 2 or 4");
    TORCH_CHECK(direct, "igemm: a subsampled residual needs a direct (stride-1) output");
    TORCH_CHECK(epi_a.has_value() && epi_a->defined() && epi_a->numel() == sub_numel,
                "igemm: subsampled residual must be [Nb][ceil(OH/2)][ceil(OW/2)][ldo]");
  }
  ConvFusion f = fusion_from(pro_sc, pro_sh, pro_seg_rows, pro_relu, 1, epi_mode, epi_a, epi_b,
                             g.C, epi_sub ? sub_numel : out.numel());
  f.epi_a_sub = epi_sub ? 1 : 0;
  if (epi_sub && epi_mode == 2)
    TORCH_CHECK(epi_b->numel() >= out.numel(), "epilogue operand b");
  f.seg_rows = (int)seg_rows;
  f.stats_seg_blocks = (int)stats_seg_blocks;
  f.stats_base = (int)stats_base;
  if (seg_rows > 0)
    TORCH_CHECK(seg_rows % bm == 0 && M % seg_rows == 0,
                "igemm: segment rows must be a multiple of the tile rows and divide M");
  if (stats_seg_blocks > 0) {
    TORCH_CHECK(has_stats && seg_rows > 0, "igemm: stats remap needs stats and seg_rows");
    const int64_t nseg = M / seg_rows;
    TORCH_CHECK(stats_base >= 0 && stats_base + seg_rows / bm <= stats_seg_blocks,
                "igemm: stats remap window out of range");
    TORCH_CHECK(stats->numel() >= nseg * stats_seg_blocks * 2 * g.N,
                "igemm: remapped stats buffer too small");
  }
  if (epi_mode == 3 || epi_mode == 4) {
    TORCH_CHECK(seg_rows > 0, "igemm mode 3/4 needs seg_rows");
    TORCH_CHECK(!f.pro_sc || epi_mode == 3 || (pro_d.has_value() && pro_d->defined()),
                "igemm: the BN-apply prologue takes epilogue mode 3 only (mode 4: BN-backward)");
    const int64_t nseg = M / seg_rows;
    f.epi_mi = optf32(epi_mi, "epi_mi");
    f.epi_S = (int)nseg;
    TORCH_CHECK(f.epi_mi && epi_mi->numel() >= 2 * nseg * g.N,
                "igemm mode 3/4: mean/invstd table must be [2][S][N]");
    if (epi_mode == 3) {
      f.epi_ss = optf32(epi_ss, "epi_ss");
      TORCH_CHECK(f.epi_ss && epi_ss->numel() >= 2 * nseg * g.N,
                  "igemm mode 3: scale/shift table must be [2][S][N]");
    } else {
      f.epi_c = optbf(epi_c, "epi_c");
      TORCH_CHECK(f.epi_c && epi_c->numel() >= out.numel(), "igemm mode 4: epilogue operand c");
      if (epi_mask.has_value() && epi_mask->defined()) {
        check_dev(*epi_mask, at::kByte, "epi_mask");
        TORCH_CHECK(epi_mask->numel() * 8 >= out.numel(), "igemm mode 4: mask size");
        f.epi_mask = epi_mask->data_ptr<uint8_t>();
      }
      if (stats2.has_value() && stats2->defined()) {
        f.stats2 = f32w(*stats2, "stats2");
        f.epi_c2 = optbf(epi_c2, "epi_c2");
        f.epi_mi2 = optf32(epi_mi2, "epi_mi2");
        TORCH_CHECK(has_stats && f.epi_c2 && f.epi_mi2 && epi_c2->numel() >= out.numel() &&
                        epi_mi2->numel() >= 2 * nseg * g.N && stats2->numel() >= stats->numel(),
                    "igemm mode 4: second BN stream needs c2, mi2 [2][S][N] and stats2");
      }
    }
  }
  if (f.pro_sc) {
    TORCH_CHECK(pro_seg_rows > 0 && pro_seg_rows % bm == 0 && M % pro_seg_rows == 0,
                "igemm prologue: segment rows must be a multiple of the tile rows");
    TORCH_CHECK(pro_sc->numel() >= (M / pro_seg_rows) * g.C, "igemm prologue: [S][C] size");
  }
  if (pro_d.has_value() && pro_d->defined()) {
    TORCH_CHECK(f.pro_sc, "igemm BN-backward prologue needs pro_sc (A) and pro_sh (B)");
    TORCH_CHECK(pro_d->numel() >= (M / pro_seg_rows) * g.C, "igemm prologue: d [S][C] size");
    TORCH_CHECK(A2.has_value() && A2->numel() == A.numel(), "igemm prologue: A2 must match A");
    TORCH_CHECK(epi_mode == 0 || epi_mode == 3 || epi_mode == 4,
                "igemm BN-backward prologue: epilogue 0, 3 or 4");
    // (igemm_patch has this prologue with the plain and mode-3 epilogues only)
    TORCH_CHECK(!(igemm_variant_patch((int)variant) && epi_mode == 4),
                "igemm BN-backward prologue on a patch variant: epilogue 0 or 3");
    f.pro_d = f32(*pro_d, "pro_d");
    f.A2 = bf(*A2, "A2");
    if (pro_out.has_value() && pro_out->defined()) {
      TORCH_CHECK(igemm_variant_patch((int)variant) && (epi_mode == 0 || epi_mode == 3),
                  "igemm: the materialised BN-backward operand (pro_out) needs a patch variant "
                  "and epilogue 0 or 3");
      TORCH_CHECK(pro_out->numel() == A.numel(), "igemm: pro_out must match A");
      const char* o0 = static_cast<const char*>(pro_out->data_ptr());
      const char* o1 = o0 + pro_out->numel() * 2;
      for (const Tensor* t : {&A, &*A2, &out}) {
        const char* t0 = static_cast<const char*>(t->data_ptr());
        const char* t1 = t0 + t->numel() * t->element_size();
        TORCH_CHECK(!(o0 < t1 && t0 < o1), "igemm: pro_out must not alias A, A2 or out");
      }
      f.pro_out = bfw(*pro_out, "pro_out");
    }
  }
  if (dual) {
    TORCH_CHECK(f.pro_sc && f.pro_sh && !f.pro_d && epi_mode == 0 && !(bias.has_value() && bias->defined()),
                "igemm block-output prologue: scale/shift tables, no other fusion");
    TORCH_CHECK(A2.has_value() && A2->numel() == A.numel(), "igemm block-output prologue: residual");
    TORCH_CHECK(pro_out->numel() == A.numel(), "igemm block-output prologue: out size");
    TORCH_CHECK(pro_mask.has_value() && pro_mask->defined() && pro_mask->numel() * 8 >= A.numel(),
                "igemm block-output prologue: mask size");
    check_dev(*pro_mask, at::kByte, "pro_mask");
    // the nb == 0 column of blocks writes relu(bn(A) + res) while the other column blocks
    // still read A / A2: the kernel applies ReLU unconditionally and the output must not alias
    TORCH_CHECK(pro_relu, "igemm block-output prologue: always applies ReLU (pro_relu required)");
    auto overlaps = [](const Tensor& a, const Tensor& b) {
      const char* a0 = static_cast<const char*>(a.data_ptr());
      const char* b0 = static_cast<const char*>(b.data_ptr());
      const char* a1 = a0 + a.numel() * a.element_size();
      const char* b1 = b0 + b.numel() * b.element_size();
      return a0 < b1 && b0 < a1;
    };
    TORCH_CHECK(!overlaps(*pro_out, A) && !overlaps(*pro_out, *A2) && !overlaps(*pro_out, out) &&
                    !overlaps(*pro_mask, A) && !overlaps(*pro_mask, *A2) && !overlaps(*pro_mask, out),
                "igemm block-output prologue: out / mask must not alias A, the residual or the "
                "conv output");
    f.A2 = bf(*A2, "A2");
    f.pro_out = bfw(*pro_out, "pro_out");
    f.pro_mask = pro_mask->data_ptr<uint8_t>();
    if (pro_rss.has_value() && pro_rss->defined()) {
      const int64_t nseg = M / pro_seg_rows;
      TORCH_CHECK(pro_rss->numel() >= 2 * nseg * g.C, "igemm block-output prologue: rss [2][S][C]");
      f.pro_rsc = f32(*pro_rss, "pro_rss");
      f.pro_rsh = f.pro_rsc + nseg * g.C;
    }
  }
  conv_igemm_nt(g, bf(A, "A"), (size_t)A.numel(), bf(B, "B"), bfw(out, "out"), optf32(bias, "bias"),
                optf32w(stats, "stats"), f, (int)variant, cur_stream());
}

int64_t igemm_bm(int64_t N) { return igemm_block_m((int)N); }
int64_t igemm_nvariants() { return igemm_num_variants(); }
int64_t igemm_vbm(int64_t v) { return igemm_variant_bm((int)v); }
int64_t igemm_vbn(int64_t v) { return igemm_variant_bn((int)v); }
bool igemm_vglds(int64_t v) { return igemm_variant_glds((int)v); }
bool igemm_gldsok(std::vector<int64_t> gv, bool pro, bool bn_bwd_pro) {
  return igemm_glds_ok(geom_from(gv), pro, bn_bwd_pro);
}
int64_t wgrad_nvariants() { return wgrad_num_variants(); }
int64_t wgrad_xlin_op(int64_t mode) { return wgrad_xlin((int)mode); }
bool wgrad_vglds(int64_t v) { return wgrad_variant_glds((int)v); }
bool igemm_vok(int64_t v, std::vector<int64_t> gv, bool pro, bool bnb, int64_t epi_mode) {
  return igemm_variant_ok((int)v, geom_from(gv), pro, bnb, (int)epi_mode);
}
bool igemm_dok(int64_t v, std::vector<int64_t> gv) { return igemm_dual_ok((int)v, geom_from(gv)); }
bool wgrad_vok(int64_t v, std::vector<int64_t> gv, bool pro, bool dpro) {
  return wgrad_variant_ok((int)v, geom_from(gv), pro, dpro);
}

int64_t wgrad_nsplit(std::vector<int64_t> gv, int64_t variant) {
  return wgrad_splits(geom_from(gv), (int)variant);
}

int64_t wgrad_ntiles(std::vector<int64_t> gv, int64_t variant) {
  return wgrad_tiles(geom_from(gv), (int)variant);
}

void wgrad(const Tensor& dY, const Tensor& X, const Tensor& partial, const Tensor& out,
           std::vector<int64_t> gv, int64_t splits, int64_t creal, double beta,
           const c10::optional<Tensor>& pro_sc, const c10::optional<Tensor>& pro_sh,
           int64_t pro_seg_rows, bool pro_relu, int64_t pro_S, int64_t variant,
           const c10::optional<Tensor>& dY2, const c10::optional<Tensor>& dp_coef,
           int64_t dp_seg_rows, int64_t dp_S) {
  const ConvGeom g = geom_from(gv);
  const int64_t M = (int64_t)g.Nb * g.OH * g.OW;
  const int64_t K = (int64_t)g.KH * g.KW * g.C;
  TORCH_CHECK(dY.numel() == M * g.N, "wgrad: dY numel mismatch");
  TORCH_CHECK(X.numel() == (int64_t)g.Nb * g.IH * g.IW * g.C, "wgrad: X numel mismatch");
  TORCH_CHECK(partial.numel() >= splits * g.N * K, "wgrad: partial too small");
  TORCH_CHECK(out.numel() == (int64_t)g.N * g.KH * g.KW * creal, "wgrad: out numel mismatch");
  TORCH_CHECK(creal <= g.C && creal > 0, "wgrad: bad creal");
  TORCH_CHECK(pro_S >= 1 && pro_S <= 2, "wgrad prologue supports at most 2 segments");
  if (variant < 0 || variant >= wgrad_num_variants()) variant = wgrad_default_variant(g.N);
  TORCH_CHECK(wgrad_variant_ok((int)variant, g, pro_sc.has_value() && pro_sc->defined(),
                               dY2.has_value() && dY2->defined()),
              "wgrad: variant ", variant, " is not admissible here: an LDS-DMA variant needs "
              "C % 64 == 0, no dY prologue, and an X prologue only on unpadded 1x1 convolutions "
              "(wgrad_pipe / wgrad_xp: none); the patch variant needs its 3x3 stride-1 geometry, "
              "N % 64 == 0 and no dY prologue");
  ConvFusion f = fusion_from(pro_sc, pro_sh, pro_seg_rows, pro_relu, pro_S, 0, c10::nullopt,
                             c10::nullopt, g.C, 0);
  if (f.pro_sc) {
    // the prologue is indexed by *input* rows, which equal output rows only for 1x1/stride-1
    TORCH_CHECK(pro_seg_rows > 0 && (int64_t)g.Nb % pro_S == 0, "wgrad prologue geometry");
  }
  if (dY2.has_value() && dY2->defined()) {
    TORCH_CHECK(dY2->numel() == dY.numel(), "wgrad: dY2 must match dY");
    TORCH_CHECK(dp_coef.has_value() && dp_coef->numel() >= 3 * dp_S * g.N, "wgrad: dp_coef [3][S][N]");
    const int64_t iters = (M + 63) / 64;
    const int64_t ips = (iters + splits - 1) / splits;
    // a split may straddle at most one segment boundary (the kernel holds two coefficient sets)
    TORCH_CHECK(dp_seg_rows > 0 && M % dp_seg_rows == 0 && M / dp_seg_rows == dp_S &&
                    (dp_S <= 2 || dp_seg_rows % (ips * 64) == 0) && dp_seg_rows % 64 == 0,
                "wgrad dY prologue: 64-row segments, and every split inside one segment when "
                "there are more than two");
    f.dY2 = bf(*dY2, "dY2");
    f.dp_coef = f32(*dp_coef, "dp_coef");
    f.dp_seg_rows = (int)dp_seg_rows;
    f.dp_S = (int)dp_S;
  }
  conv_wgrad(g, bf(dY, "dY"), bf(X, "X"), (size_t)X.numel(), f32w(partial, "partial"), (int)splits,
             f32w(out, "out"), (int)creal, (float)beta, f, (int)variant, cur_stream());
}


// fused 1x1 backward of a bottleneck conv3 (conv.hip conv1x1_bwd_dual): returns nothing; writes
// gm [M][Ci], stats [S*bps][2][Ci] (BN2-backward partials), wpart [S*bps][Co][Ci] (dW slabs)
void conv1x1_bwd_dual_op(const Tensor& G, const c10::optional<Tensor>& A3,
                         const c10::optional<Tensor>& coef, const Tensor& X,
                         const c10::optional<Tensor>& xss, const c10::optional<Tensor>& xmi,
                         const Tensor& Wt, const Tensor& gm,
                         const Tensor& stats, const Tensor& wpart, int64_t S, int64_t bps,
                         const c10::optional<Tensor>& Xraw, bool dual8) {
  const int64_t CI = gm.size(-1);
  const int64_t M = gm.numel() / CI;
  const int64_t CO = G.numel() / M;
  const uint16_t* xr = optbf(Xraw, "Xraw");
  TORCH_CHECK((CO == 256 && CI == 64 && xr == nullptr) || (CO == 512 && CI == 128),
              "conv1x1_bwd_dual: (Co, Ci) = (256, 64) or (512, 128); a pre-applied X (Xraw "
              "given) only with (512, 128)");
  if (xr != nullptr) TORCH_CHECK(Xraw->numel() == M * CI, "conv1x1_bwd_dual: Xraw size");
  TORCH_CHECK(G.numel() == M * CO && X.numel() == M * CI && Wt.numel() == CI * CO,
              "conv1x1_bwd_dual: operand sizes");
  TORCH_CHECK(S >= 1 && S <= 2 && bps >= 1 && M % S == 0 && (M / S) % (64 * bps) == 0,
              "conv1x1_bwd_dual: every block's rows must lie in one segment (64-row tiles)");
  const float* xs = optf32(xss, "xss");
  const float* xm = optf32(xmi, "xmi");
  // no BN2 tables: the plain form (a downsample conv; no mask, no partials) — (256, 64) only
  TORCH_CHECK((xs == nullptr) == (xm == nullptr), "conv1x1_bwd_dual: xss and xmi together");
  TORCH_CHECK(xs != nullptr || (CO == 256 && CI == 64 && xr == nullptr),
              "conv1x1_bwd_dual: the plain form is (Co, Ci) = (256, 64) only");
  if (xs != nullptr) {
    TORCH_CHECK(xss->numel() >= 2 * S * CI && xmi->numel() >= 2 * S * CI,
                "conv1x1_bwd_dual: BN2 tables");
    TORCH_CHECK(stats.numel() >= S * bps * 2 * CI, "conv1x1_bwd_dual: stats size");
  }
  TORCH_CHECK(wpart.numel() >= S * bps * CO * CI, "conv1x1_bwd_dual: wpart size");
  TORCH_CHECK(M * CO * 2 < (int64_t(1) << 31), "conv1x1_bwd_dual: 32-bit buffer offsets");
  const uint16_t* a3 = optbf(A3, "A3");
  const float* cf = optf32(coef, "coef");
  if (a3 != nullptr) {
    TORCH_CHECK(A3->numel() == G.numel() && cf != nullptr && coef->numel() >= 3 * S * CO,
                "conv1x1_bwd_dual: lazy BN-backward needs A3 [M][Co] and coef [3][S][Co]");
  }
  conv1x1_bwd_dual(bf(G, "G"), a3, cf, bf(X, "X"), xs, xm,
                   bf(Wt, "Wt"), bfw(gm, "gm"), f32w(stats, "stats"), f32w(wpart, "wpart"),
                   (int)M, (int)CO, (int)CI, (int)S, (int)bps, cur_stream(), xr, dual8);
}

// 1x1 stride-2 downsample backward (layer2.0): X [N][H][W][Ci] block input, gm [N][OH][OW][Ci]
void conv1x1_bwd_dual_s2_op(const Tensor& G, const c10::optional<Tensor>& A3,
                            const c10::optional<Tensor>& coef, const Tensor& X, const Tensor& Wt,
                            const Tensor& gm, const Tensor& wpart, int64_t S, int64_t bps) {
  TORCH_CHECK(X.dim() == 4 && gm.dim() == 4, "conv1x1_bwd_dual_s2: NHWC 4-D X and gm");
  const int64_t N = X.size(0), H = X.size(1), W = X.size(2), CI = X.size(3);
  const int64_t OH = gm.size(1), OW = gm.size(2);
  TORCH_CHECK(gm.size(0) == N && gm.size(3) == CI && OH == (H + 1) / 2 && OW == (W + 1) / 2,
              "conv1x1_bwd_dual_s2: gm is the stride-2 output map");
  const int64_t Mo = N * OH * OW;
  const int64_t CO = G.numel() / Mo;
  TORCH_CHECK(CO == 512 && CI == 256 && G.numel() == Mo * CO && Wt.numel() == CI * CO,
              "conv1x1_bwd_dual_s2: (Co, Ci) = (512, 256) only");
  TORCH_CHECK(S >= 1 && S <= 2 && N % S == 0 && bps >= 1 && (Mo / S) % (64 * bps) == 0,
              "conv1x1_bwd_dual_s2: every block's rows must lie in one segment");
  TORCH_CHECK(wpart.numel() >= S * bps * CO * CI, "conv1x1_bwd_dual_s2: wpart size");
  TORCH_CHECK(Mo * CO * 2 < (int64_t(1) << 31) && X.numel() * 2 < (int64_t(1) << 31),
              "conv1x1_bwd_dual_s2: 32-bit buffer offsets");
  const uint16_t* a3 = optbf(A3, "A3");
  const float* cf = optf32(coef, "coef");
  TORCH_CHECK(a3 == nullptr && cf == nullptr,
              "conv1x1_bwd_dual_s2: dY must be materialised (no lazy BN-backward form)");
  conv1x1_bwd_dual_s2(bf(G, "G"), a3, cf, bf(X, "X"), bf(Wt, "Wt"), bfw(gm, "gm"),
                      f32w(wpart, "wpart"), (int)Mo, (int)CO, (int)CI, (int)S, (int)bps, (int)H,
                      (int)W, (int)OH, (int)OW, cur_stream());
}

void wgrad_reduce_slabs_op(const Tensor& partial, int64_t splits, const Tensor& out, double beta) {
  const int64_t n = out.numel();
  TORCH_CHECK(n % 4 == 0 && partial.numel() >= splits * n && splits >= 1,
              "wgrad_reduce_slabs: sizes");
  wgrad_reduce_slabs(f32w(partial, "partial"), (int)splits, f32w(out, "out"), (size_t)n,
                     (float)beta, cur_stream());
}

void weight_transform(const Tensor& W, const Tensor& Wt, std::vector<int64_t> p) {
  TORCH_CHECK(p.size() == 10, "weight_transform params");
  const int Co = p[0], KH = p[1], KW = p[2], Ci = p[3], KHs = p[4], KWs = p[5];
  TORCH_CHECK(W.numel() == (int64_t)Co * KH * KW * Ci, "weight_transform: W numel");
  TORCH_CHECK(Wt.numel() == (int64_t)Ci * KHs * KWs * Co, "weight_transform: Wt numel");
  for (int a = 0; a < KHs; ++a) {
    const int kh = (int)p[6] + a * (int)p[7];
    TORCH_CHECK(kh >= 0 && kh < KH, "weight_transform: kh out of range");
  }
  for (int a = 0; a < KWs; ++a) {
    const int kw = (int)p[8] + a * (int)p[9];
    TORCH_CHECK(kw >= 0 && kw < KW, "weight_transform: kw out of range");
  }
  conv_weight_transform(bf(W, "W"), bfw(Wt, "Wt"), Co, KH, KW, Ci, KHs, KWs, p[6], p[7], p[8], p[9],
                        cur_stream());
}

// Batched dgrad weight transforms: plan (validate + device descriptor table, eager) and launch.
// The plan holds raw pointers: the caller keeps every W / Wt tensor alive and unmoved while
// it is used (FusedStages caches it next to the tensors and rebuilds it when they change).
Tensor weight_transform_plan(const std::vector<Tensor>& Ws, const std::vector<Tensor>& Wts,
                             std::vector<int64_t> p) {
  const size_t n = Ws.size();
  TORCH_CHECK(n > 0 && Wts.size() == n && p.size() == 10 * n, "weight_transform_plan sizes");
  Tensor host = at::empty({(int64_t)(n * sizeof(WtDesc) / 8) + 1},
                          at::TensorOptions().dtype(at::kLong));
  WtDesc* d = reinterpret_cast<WtDesc*>(host.data_ptr<int64_t>());
  int blk = 0;
  for (size_t i = 0; i < n; ++i) {
    const int64_t* q = p.data() + 10 * i;
    const int Co = q[0], KH = q[1], KW = q[2], Ci = q[3], KHs = q[4], KWs = q[5];
    TORCH_CHECK(Ws[i].numel() == (int64_t)Co * KH * KW * Ci, "weight_transform_plan: W numel");
    TORCH_CHECK(Wts[i].numel() == (int64_t)Ci * KHs * KWs * Co, "weight_transform_plan: Wt numel");
    TORCH_CHECK(Ws[i].device() == Wts[0].device() && Wts[i].device() == Wts[0].device(),
                "weight_transform_plan: one device");
    for (int a = 0; a < KHs; ++a)
      TORCH_CHECK(q[6] + a * q[7] >= 0 && q[6] + a * q[7] < KH, "weight_transform_plan: kh");
    for (int a = 0; a < KWs; ++a)
      TORCH_CHECK(q[8] + a * q[9] >= 0 && q[8] + a * q[9] < KW, "weight_transform_plan: kw");
    const int nb = ((Co + 63) / 64) * ((Ci + 63) / 64) * KHs * KWs;  // 64x64 tiles per tap
    d[i] = WtDesc{bf(Ws[i], "W"), bfw(Wts[i], "Wt"), Co, KH, KW, Ci, KHs, KWs, (int)q[6],
                  (int)q[7], (int)q[8], (int)q[9], blk, nb};
    blk += nb;
  }
  // host table [n descriptors | total block count]; the caller moves the descriptors to the
  // device once and keeps the count on the host (no sync per launch, graph-capturable)
  host.data_ptr<int64_t>()[n * sizeof(WtDesc) / 8] = blk;
  return host;
}

void weight_transform_batch(const Tensor& table, int64_t total_blocks) {
  TORCH_CHECK(table.is_cuda() && table.scalar_type() == at::kLong && table.numel() % 8 == 0 &&
                  table.numel() > 0 && total_blocks > 0,
              "weight_transform_batch: device descriptors from weight_transform_plan");
  conv_weight_transform_batch(reinterpret_cast<const WtDesc*>(table.data_ptr<int64_t>()),
                              (int)(table.numel() / 8), (int)total_blocks, cur_stream());
}

// ------------------------------------------------------------------------------- batch norm
void check_rc(const Tensor& x, int64_t S, const char* n) {
  TORCH_CHECK(x.dim() >= 2, n, ": rank");
  const int64_t C = x.size(-1);
  TORCH_CHECK(C % 8 == 0, n, ": channels must be a multiple of 8");
  const int64_t CH = C / 8;
  TORCH_CHECK(CH <= 256 || CH % 256 == 0, n, ": unsupported channel count");
  TORCH_CHECK((x.numel() / C) % S == 0, n, ": rows not divisible by segments");
}

int64_t bn_blocks(int64_t R, int64_t C, int64_t S) {
  return bn_stats_blocks_per_seg((int)R, (int)C, (int)S);
}

void bn_stats(const Tensor& x, int64_t S, const Tensor& partial) {
  check_rc(x, S, "bn_stats");
  const int C = x.size(-1), R = x.numel() / C;
  const int nblk = bn_stats_blocks_per_seg(R, C, S);
  TORCH_CHECK(partial.numel() >= (int64_t)S * nblk * 2 * C, "bn_stats: partial too small");
  bn_stats_partial(bf(x, "x"), R, C, S, f32w(partial, "partial"), nullptr, cur_stream());
}

void bn_reduce(const Tensor& partial, int64_t nblk, int64_t S, int64_t C, const Tensor& stats) {
  TORCH_CHECK(partial.numel() >= S * nblk * 2 * C && stats.numel() >= 2 * S * C, "bn_reduce sizes");
  const int G = bn_reduce_groups((int)nblk);
  TORCH_CHECK(G == 1 || C % 4 == 0, "bn_reduce: C must be a multiple of 4 (float4 partial rows)");
  at::Tensor ws;
  float* wsp = nullptr;
  if (G > 1) {
    ws = at::empty({S * G * 2 * C}, stats.options());
    wsp = ws.data_ptr<float>();
  }
  bn_reduce_partials(f32(partial, "partial"), nblk, S, C, f32w(stats, "stats"), wsp, cur_stream());
}

void bn_final(const Tensor& stats, int64_t S, int64_t C, double count, double eps, double momentum,
              const c10::optional<Tensor>& rm, const c10::optional<Tensor>& rv, const Tensor& mi,
              const c10::optional<Tensor>& nbt, const c10::optional<Tensor>& gamma,
              const c10::optional<Tensor>& beta, const c10::optional<Tensor>& ss) {
  if (ss.has_value() && ss->defined()) TORCH_CHECK(ss->numel() >= 2 * S * C, "bn_finalize: ss size");
  if (gamma.has_value() && gamma->defined()) TORCH_CHECK(gamma->numel() == C, "bn_finalize: gamma");
  if (beta.has_value() && beta->defined()) TORCH_CHECK(beta->numel() == C, "bn_finalize: beta");
  TORCH_CHECK(stats.numel() >= 2 * S * C && mi.numel() >= 2 * S * C, "bn_finalize sizes");
  int64_t* nb = nullptr;
  if (nbt.has_value() && nbt->defined()) {
    check_dev(*nbt, at::kLong, "num_batches_tracked");
    nb = nbt->data_ptr<int64_t>();
  }
  bn_finalize(f32(stats, "stats"), S, C, (float)count, (float)eps, (float)momentum,
              optf32w(rm, "running_mean"), optf32w(rv, "running_var"), f32w(mi, "mean_invstd"), nb,
              optf32(gamma, "gamma"), optf32(beta, "beta"), optf32w(ss, "ss"), cur_stream());
}

// persistent zeroed ticket arrays for the last-arriver reductions, per device and per slot:
// reductions that may run concurrently (different streams) must use different slots
constexpr int kTicketSlots = 4;  // 0/1 BN reduce per stream, 2/3 conv tails per stream
constexpr int64_t kTicketStride = 4096;
unsigned* tickets_for(const Tensor& like, int64_t n, int64_t slot) {
  static std::vector<Tensor> per_dev;
  TORCH_CHECK(slot >= 0 && slot < kTicketSlots, "ticket slot out of range");
  TORCH_CHECK(n <= kTicketStride, "too many channel groups for the ticket array");
  const int d = like.get_device();
  if ((int)per_dev.size() <= d) per_dev.resize(d + 1);
  if (!per_dev[d].defined()) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    (void)hipStreamIsCapturing(cur_stream(), &cs);
    TORCH_CHECK(cs == hipStreamCaptureStatusNone,
                "bn ticket array must be allocated before graph capture");
    per_dev[d] = at::zeros({kTicketSlots * kTicketStride}, like.options().dtype(at::kInt));
  }
  return reinterpret_cast<unsigned*>(per_dev[d].data_ptr<int>()) + slot * kTicketStride;
}

void bn_reduce_fused_op(const Tensor& partial, int64_t nblk, int64_t S, int64_t C, int64_t mode,
                        const c10::optional<Tensor>& stats, double count, double eps,
                        double momentum, const c10::optional<Tensor>& rm,
                        const c10::optional<Tensor>& rv, const c10::optional<Tensor>& mi,
                        const c10::optional<Tensor>& nbt, const c10::optional<Tensor>& gamma,
                        const c10::optional<Tensor>& beta, const c10::optional<Tensor>& ss,
                        const c10::optional<Tensor>& dgamma, const c10::optional<Tensor>& dbeta,
                        const c10::optional<Tensor>& coef, int64_t ticket_slot,
                        const c10::optional<Tensor>& ipc_peers,
                        const c10::optional<Tensor>& ipc_arena, int64_t ipc_site,
                        const c10::optional<Tensor>& ipc_epoch,
                        const c10::optional<Tensor>& ipc_err, int64_t world, int64_t rank) {
  TORCH_CHECK(mode >= 0 && mode <= 2, "bn_reduce_fused: mode");
  TORCH_CHECK(nblk > 0 && partial.numel() >= S * nblk * 2 * C, "bn_reduce_fused: partial size");
  TORCH_CHECK(C % 4 == 0, "bn_reduce_fused: C must be a multiple of 4 (float4 partial rows)");
  TORCH_CHECK(S >= 1 && S <= 4, "bn_reduce_fused: at most 4 segments");
  BnReduceFusedParams q;
  q.partial = f32(partial, "partial");
  q.nblk = (int)nblk; q.S = (int)S; q.C = (int)C; q.mode = (int)mode;
  const int G = bn_reduce_groups((int)nblk);
  at::Tensor ws = at::empty({S * G * 2 * C}, partial.options());
  q.ws = ws.data_ptr<float>();
  q.tickets = tickets_for(partial, (C + 63) / 64, ticket_slot);
  q.count = (float)count; q.eps = (float)eps; q.momentum = (float)momentum;
  if (mode == 0) {
    TORCH_CHECK(stats.has_value() && stats->numel() >= 2 * S * C, "bn_reduce_fused: stats");
    q.stats = f32w(*stats, "stats");
    // optional: the local dβ = Σ_s Σg, dγ = Σ_s Σg·x̂ of a BatchNorm backward's partials (the
    // distributed path all-reduces `stats` for the input-gradient coefficients afterwards)
    q.dgamma = optf32w(dgamma, "dgamma");
    q.dbeta = optf32w(dbeta, "dbeta");
  } else if (mode == 1) {
    TORCH_CHECK(mi.has_value() && mi->numel() >= 2 * S * C, "bn_reduce_fused: mi");
    q.mi = f32w(*mi, "mi");
    q.running_mean = optf32w(rm, "running_mean");
    q.running_var = optf32w(rv, "running_var");
    if (nbt.has_value() && nbt->defined()) {
      check_dev(*nbt, at::kLong, "num_batches_tracked");
      q.nbt = nbt->data_ptr<int64_t>();
    }
    q.gamma = optf32(gamma, "gamma");
    q.beta = optf32(beta, "beta");
    if (ss.has_value() && ss->defined()) TORCH_CHECK(ss->numel() >= 2 * S * C, "bn_reduce_fused: ss");
    q.ss = optf32w(ss, "ss");
  } else {
    TORCH_CHECK(mi.has_value() && mi->numel() >= 2 * S * C, "bn_reduce_fused: mi");
    TORCH_CHECK(coef.has_value() && coef->numel() >= 3 * S * C, "bn_reduce_fused: coef");
    q.mi = const_cast<float*>(f32(*mi, "mi"));
    q.gamma = optf32(gamma, "gamma");
    q.dgamma = optf32w(dgamma, "dgamma");
    q.dbeta = optf32w(dbeta, "dbeta");
    q.coef = f32w(*coef, "coef");
  }
  if (q.gamma) TORCH_CHECK(gamma->numel() == C, "bn_reduce_fused: gamma size");
  if (q.beta) TORCH_CHECK(beta->numel() == C, "bn_reduce_fused: beta size");
  if (q.dgamma) TORCH_CHECK(dgamma->numel() == C, "bn_reduce_fused: dgamma size");
  if (q.dbeta) TORCH_CHECK(dbeta->numel() == C, "bn_reduce_fused: dbeta size");
  if (world > 1) {
    // IPC statistics exchange (bn.hip bn_ipc_exchange): every rank's arena must hold this
    // site's region, the peer table one base per rank, the epochs one counter per channel group
    TORCH_CHECK(mode == 1 || mode == 2, "bn_reduce_fused: the IPC exchange finalizes (mode 1/2)");
    TORCH_CHECK(world <= 16 && rank >= 0 && rank < world, "bn_reduce_fused: world / rank");
    TORCH_CHECK(ipc_peers.has_value() && ipc_arena.has_value() && ipc_epoch.has_value() &&
                    ipc_err.has_value(), "bn_reduce_fused: IPC exchange needs peers, arena, epoch, err");
    check_dev(*ipc_peers, at::kLong, "ipc_peers");
    check_dev(*ipc_arena, at::kLong, "ipc_arena");
    check_dev(*ipc_epoch, at::kInt, "ipc_epoch");
    check_dev(*ipc_err, at::kInt, "ipc_err");
    TORCH_CHECK(ipc_peers->numel() == world, "bn_reduce_fused: peer table size");
    TORCH_CHECK(ipc_epoch->numel() >= (C + 63) / 64, "bn_reduce_fused: epoch counters");
    TORCH_CHECK(ipc_site >= 0 && ipc_site + bn_ipc_region_words((int)world, (int)S, (int)C) <=
                                    ipc_arena->numel(),
                "bn_reduce_fused: IPC site region outside the arena");
    q.ipc_peers = reinterpret_cast<uint64_t* const*>(ipc_peers->data_ptr<int64_t>());
    q.ipc_own = reinterpret_cast<uint64_t*>(ipc_arena->data_ptr<int64_t>());
    q.ipc_site = ipc_site;
    q.ipc_epoch = reinterpret_cast<unsigned*>(ipc_epoch->data_ptr<int>());
    q.ipc_err = ipc_err->data_ptr<int>();
    q.world = (int)world;
    q.rank = (int)rank;
  }
  bn_reduce_fused(q, cur_stream());
}

// one-shot IPC all-gather (op 0: dst [W][n] <- every rank's src [n]) or reduce-scatter (op 1:
// dst [n] <- sum over ranks of src [W][n] row `rank`) of 32-bit words (comm.hip)
void ipc_collective_op(int64_t op, const Tensor& src, const Tensor& dst, const Tensor& peers,
                       const Tensor& arena, int64_t site, const Tensor& epoch, const Tensor& err,
                       int64_t world, int64_t rank) {
  TORCH_CHECK(op == 0 || op == 1, "ipc_collective: op 0 (all-gather) or 1 (reduce-scatter)");
  const bool words = src.element_size() == 4 && dst.element_size() == 4;
  const bool pairs = op == 0 && src.element_size() == 2 && dst.element_size() == 2;
  TORCH_CHECK(src.is_cuda() && dst.is_cuda() && src.is_contiguous() && dst.is_contiguous() &&
                  (words || pairs),
              "ipc_collective: contiguous 32-bit (or bf16 pairs for the all-gather) GPU tensors");
  const int64_t nbytes = src.numel() * src.element_size();
  TORCH_CHECK(nbytes % 4 == 0, "ipc_collective: payload must be whole 32-bit words");
  const int64_t n = op == 0 ? nbytes / 4 : nbytes / 4 / world;
  TORCH_CHECK(world >= 1 && world <= 16 && rank >= 0 && rank < world, "ipc_collective: world");
  TORCH_CHECK(dst.numel() * dst.element_size() == (op == 0 ? world * n * 4 : n * 4),
              "ipc_collective: dst size");
  TORCH_CHECK(op == 0 || src.numel() * src.element_size() == world * n * 4,
              "ipc_collective: reduce-scatter src must be [world][n] words");
  check_dev(peers, at::kLong, "ipc_peers");
  check_dev(arena, at::kLong, "ipc_arena");
  check_dev(epoch, at::kInt, "ipc_epoch");
  check_dev(err, at::kInt, "ipc_err");
  TORCH_CHECK(peers.numel() == world, "ipc_collective: peer table size");
  TORCH_CHECK(epoch.numel() >= IPC_COLL_BLOCKS, "ipc_collective: epoch counters");
  TORCH_CHECK(site >= 0 && site + ipc_coll_region_words((int)world, (int)n) <= arena.numel(),
              "ipc_collective: site outside the arena");
  ipc_collective((int)op, static_cast<const uint32_t*>(src.data_ptr()),
                 static_cast<uint32_t*>(dst.data_ptr()), (int)n,
                 reinterpret_cast<uint64_t* const*>(peers.data_ptr<int64_t>()),
                 reinterpret_cast<uint64_t*>(arena.data_ptr<int64_t>()), site,
                 reinterpret_cast<unsigned*>(epoch.data_ptr<int>()), err.data_ptr<int>(),
                 (int)world, (int)rank, cur_stream());
}

void bn_apply_ss_op(const Tensor& x, const Tensor& ss, const c10::optional<Tensor>& res,
                    const c10::optional<Tensor>& rss, const Tensor& y, int64_t S, bool relu,
                    const c10::optional<Tensor>& mask) {
  check_rc(x, S, "bn_apply_ss");
  const int C = x.size(-1), R = x.numel() / C;
  TORCH_CHECK(y.numel() == x.numel(), "bn_apply_ss: y size");
  TORCH_CHECK(ss.numel() >= 2 * S * C, "bn_apply_ss: ss size");
  const bool has_res = res.has_value() && res->defined();
  if (has_res) TORCH_CHECK(res->numel() == x.numel(), "bn_apply_ss: res size");
  if (rss.has_value() && rss->defined())
    TORCH_CHECK(has_res && rss->numel() >= 2 * S * C, "bn_apply_ss: rss needs res, [2][S][C]");
  uint8_t* mk = nullptr;
  if (mask.has_value() && mask->defined()) {
    check_dev(*mask, at::kByte, "mask");
    TORCH_CHECK(mask->numel() * 8 == x.numel(), "bn_apply_ss: mask must be [R][C/8] uint8");
    mk = mask->data_ptr<uint8_t>();
  }
  bn_apply_ss(bf(x, "x"), f32(ss, "ss"), optbf(res, "res"), optf32(rss, "rss"), bfw(y, "y"), mk, R,
              C, S, relu ? 1 : 0, cur_stream());
}

void bn_apply_op(const Tensor& x, const c10::optional<Tensor>& res, const Tensor& y,
                 const Tensor& mi, const c10::optional<Tensor>& gamma,
                 const c10::optional<Tensor>& beta, int64_t S, bool relu) {
  check_rc(x, S, "bn_apply");
  const int C = x.size(-1), R = x.numel() / C;
  TORCH_CHECK(y.numel() == x.numel(), "bn_apply: y size");
  if (res.has_value() && res->defined()) TORCH_CHECK(res->numel() == x.numel(), "bn_apply: res size");
  TORCH_CHECK(mi.numel() >= 2 * S * C, "bn_apply: mean_invstd size");
  bn_apply(bf(x, "x"), optbf(res, "res"), bfw(y, "y"), f32(mi, "mi"), optf32(gamma, "gamma"),
           optf32(beta, "beta"), R, C, S, relu ? 1 : 0, cur_stream());
}

void bn_apply_eval_op(const Tensor& x, const c10::optional<Tensor>& res, const Tensor& y,
                      const Tensor& rm, const Tensor& rv, const c10::optional<Tensor>& gamma,
                      const c10::optional<Tensor>& beta, double eps, bool relu) {
  check_rc(x, 1, "bn_apply_eval");
  const int C = x.size(-1), R = x.numel() / C;
  TORCH_CHECK(y.numel() == x.numel(), "bn_apply_eval: y size");
  bn_apply_eval(bf(x, "x"), optbf(res, "res"), bfw(y, "y"), f32(rm, "rm"), f32(rv, "rv"),
                optf32(gamma, "gamma"), optf32(beta, "beta"), (float)eps, R, C, relu ? 1 : 0,
                cur_stream());
}

void bn_bwd_reduce_op(const Tensor& dy, const c10::optional<Tensor>& y, const Tensor& x,
                      const Tensor& mi, int64_t S, bool relu, const Tensor& partial) {
  check_rc(x, S, "bn_bwd_reduce");
  const int C = x.size(-1), R = x.numel() / C;
  TORCH_CHECK(dy.numel() == x.numel(), "bn_bwd_reduce: dy size");
  TORCH_CHECK(!relu || (y.has_value() && y->numel() == x.numel()), "bn_bwd_reduce: y needed");
  const int nblk = bn_stats_blocks_per_seg(R, C, S);
  TORCH_CHECK(partial.numel() >= (int64_t)S * nblk * 2 * C, "bn_bwd_reduce: partial too small");
  bn_bwd_reduce(bf(dy, "dy"), optbf(y, "y"), bf(x, "x"), f32(mi, "mi"), R, C, S, relu ? 1 : 0,
                f32w(partial, "partial"), cur_stream());
}

void bn_bwd_final(const Tensor& sums, const Tensor& mi, const c10::optional<Tensor>& gamma,
                  int64_t S, int64_t C, double count, const c10::optional<Tensor>& dgamma,
                  const c10::optional<Tensor>& dbeta, const Tensor& coef) {
  TORCH_CHECK(sums.numel() >= 2 * S * C && coef.numel() >= 3 * S * C, "bn_bwd_finalize sizes");
  bn_bwd_finalize(f32(sums, "sums"), f32(mi, "mi"), optf32(gamma, "gamma"), S, C, (float)count,
                  optf32w(dgamma, "dgamma"), optf32w(dbeta, "dbeta"), f32w(coef, "coef"),
                  cur_stream());
}

void bn_bwd_apply_op(const Tensor& dy, const c10::optional<Tensor>& y, const Tensor& x,
                     const Tensor& coef, int64_t S, bool relu, const Tensor& dx,
                     const c10::optional<Tensor>& dres) {
  check_rc(x, S, "bn_bwd_apply");
  const int C = x.size(-1), R = x.numel() / C;
  TORCH_CHECK(dy.numel() == x.numel() && dx.numel() == x.numel(), "bn_bwd_apply sizes");
  TORCH_CHECK(!relu || (y.has_value() && y->numel() == x.numel()), "bn_bwd_apply: y needed");
  bn_bwd_apply(bf(dy, "dy"), optbf(y, "y"), bf(x, "x"), f32(coef, "coef"), R, C, S, relu ? 1 : 0,
               bfw(dx, "dx"), optbfw(dres, "dres"), cur_stream());
}

void bn_bwd_apply2_op(const Tensor& g, const Tensor& x1, const Tensor& coef1, const Tensor& dx1,
                      const Tensor& x2, const Tensor& coef2, const Tensor& dx2, int64_t S) {
  check_rc(x1, S, "bn_bwd_apply2");
  const int C = x1.size(-1), R = x1.numel() / C;
  TORCH_CHECK(g.numel() == x1.numel() && x2.numel() == x1.numel() && dx1.numel() == x1.numel() &&
                  dx2.numel() == x1.numel(), "bn_bwd_apply2 sizes");
  TORCH_CHECK(coef1.numel() >= 3 * S * C && coef2.numel() >= 3 * S * C, "bn_bwd_apply2 coef");
  bn_bwd_apply2(bf(g, "g"), bf(x1, "x1"), f32(coef1, "coef1"), bfw(dx1, "dx1"), bf(x2, "x2"),
                f32(coef2, "coef2"), bfw(dx2, "dx2"), R, C, S, cur_stream());
}

// ------------------------------------------------------------------------------- misc
void avgpool_fwd_op(const Tensor& x, const Tensor& y, int64_t Nb, int64_t HW, int64_t C) {
  TORCH_CHECK(C % 8 == 0 && x.numel() == Nb * HW * C && y.numel() == Nb * C, "avgpool_fwd sizes");
  avgpool_fwd(bf(x, "x"), bfw(y, "y"), Nb, HW, C, cur_stream());
}
void avgpool_bwd_op(const Tensor& dy, const Tensor& dx, int64_t Nb, int64_t HW, int64_t C) {
  TORCH_CHECK(C % 8 == 0 && dx.numel() == Nb * HW * C && dy.numel() == Nb * C, "avgpool_bwd sizes");
  avgpool_bwd(bf(dy, "dy"), bfw(dx, "dx"), Nb, HW, C, cur_stream());
}
void colsum_op(const Tensor& x, const Tensor& out, double beta) {
  const int C = x.size(-1), R = x.numel() / C;
  TORCH_CHECK(out.numel() == C, "colsum sizes");
  at::Tensor ws = at::empty({(int64_t)colsum_groups(R) * C}, out.options());
  colsum_bf16(bf(x, "x"), R, C, f32w(out, "out"), (float)beta, ws.data_ptr<float>(), cur_stream());
}
void cast_to_bf16(const Tensor& x, const Tensor& y) {
  TORCH_CHECK(x.numel() == y.numel(), "cast sizes");
  cast_f32_bf16(f32(x, "x"), bfw(y, "y"), x.numel(), cur_stream());
}
void cast_to_f32(const Tensor& x, const Tensor& y) {
  TORCH_CHECK(x.numel() == y.numel(), "cast sizes");
  cast_bf16_f32(bf(x, "x"), f32w(y, "y"), x.numel(), cur_stream());
}

// ------------------------------------------------------------------------------- nt-xent
void nt_normalize(const Tensor& z, const Tensor& zn, const Tensor& inv_norm) {
  TORCH_CHECK(z.dim() == 2, "nt_normalize: z must be 2-D");
  const int R = z.size(0), D = z.size(1);
  TORCH_CHECK(zn.numel() == (int64_t)R * D && inv_norm.numel() == R, "nt_normalize sizes");
  ntxent_normalize_f32(bf(z, "z"), R, D, f32w(zn, "zn"), f32w(inv_norm, "inv_norm"), cur_stream());
}
void nt_transpose(const Tensor& in, const Tensor& out) {
  const int R = in.size(0), D = in.size(1);
  TORCH_CHECK(out.numel() == (int64_t)R * D, "nt_transpose sizes");
  ntxent_transpose(f32(in, "in"), f32w(out, "out"), R, D, cur_stream());
}
void check_nt(int R, int Ccols, int D, int col_offset, int n_local) {
  TORCH_CHECK(R % 16 == 0 && Ccols % 16 == 0, "ntxent: rows/cols must be multiples of 16");
  TORCH_CHECK(D == 32 || D == 64 || D == 128 || D == 256, "ntxent: D must be 32/64/128/256");
  TORCH_CHECK(2 * n_local == R, "ntxent: R must be 2*n_local");
  TORCH_CHECK(col_offset >= 0 && col_offset + R <= Ccols, "ntxent: bad col_offset");
}
int64_t nt_fwd_splits(int64_t R, int64_t C) { return ntxent_fwd_splits(R, C); }
// rows [R][D] -> columns [c0, c0 + R) of out [D][Ccols]
void nt_transpose_cols(const Tensor& in, const Tensor& out, int64_t c0) {
  const int R = in.size(0), D = in.size(1);
  TORCH_CHECK(out.dim() == 2 && out.size(0) == D && c0 >= 0 && c0 + R <= out.size(1),
              "nt_transpose_cols: out must be [D][Ccols] with room for columns [c0, c0 + R)");
  ntxent_transpose_cols(f32(in, "in"), f32w(out, "out"), R, D, (int)out.size(1), (int)c0,
                        cur_stream());
}
// forward partials of columns [c_lo, c_hi) into splits [split_base, split_base + splits)
void nt_forward_range(const Tensor& znT, int64_t R, int64_t col_offset, int64_t n_local,
                      double inv_temp, const Tensor& part, int64_t c_lo, int64_t c_hi,
                      int64_t splits, int64_t split_base) {
  const int D = znT.size(0), Ccols = znT.size(1);
  check_nt(R, Ccols, D, col_offset, n_local);
  TORCH_CHECK(c_lo >= 0 && c_lo < c_hi && c_hi <= Ccols && c_lo % 16 == 0 && c_hi % 16 == 0 &&
                  splits >= 1 && split_base >= 0 && part.numel() >= (split_base + splits) * R * 3,
              "nt_forward_range: column window / splits");
  ntxent_forward_range(f32(znT, "znT"), R, Ccols, D, col_offset, n_local, (float)inv_temp,
                       f32w(part, "part"), c_lo, c_hi, splits, split_base, cur_stream());
}
void nt_finish(const Tensor& part, int64_t R, int64_t splits, const Tensor& lse,
               const Tensor& loss) {
  TORCH_CHECK(part.numel() >= splits * R * 3 && lse.numel() == R && loss.numel() == R,
              "nt_finish sizes");
  ntxent_finish(f32(part, "part"), R, splits, f32w(lse, "lse"), f32w(loss, "loss"), cur_stream());
}
int64_t nt_bwd_splits(int64_t nown, int64_t npart) { return ntxent_bwd_splits(nown, npart); }
void nt_forward(const Tensor& znT, int64_t R, int64_t col_offset, int64_t n_local, double inv_temp,
                const Tensor& part, int64_t splits, const Tensor& lse, const Tensor& loss) {
  const int D = znT.size(0), Ccols = znT.size(1);
  check_nt(R, Ccols, D, col_offset, n_local);
  TORCH_CHECK(part.numel() >= splits * R * 3 && lse.numel() == R && loss.numel() == R,
              "nt_forward sizes");
  ntxent_forward(f32(znT, "znT"), R, Ccols, D, col_offset, n_local, (float)inv_temp,
                 f32w(part, "part"), splits, f32w(lse, "lse"), f32w(loss, "loss"), cur_stream());
}
void nt_backward_part(bool row_mode, const Tensor& zn, const Tensor& znT, const Tensor& lse,
                      int64_t R, int64_t col_offset, int64_t n_local, double inv_temp,
                      double gscale, const c10::optional<Tensor>& gout, const Tensor& part,
                      int64_t splits, const Tensor& out) {
  const int D = znT.size(0), Ccols = znT.size(1);
  check_nt(R, Ccols, D, col_offset, n_local);
  TORCH_CHECK(zn.numel() == (int64_t)Ccols * D, "nt_backward: zn size");
  const int64_t nown = row_mode ? R : Ccols;
  TORCH_CHECK(part.numel() >= splits * nown * D && out.numel() == nown * D, "nt_backward sizes");
  ntxent_backward_part(row_mode ? 1 : 0, f32(zn, "zn"), f32(znT, "znT"), f32(lse, "lse"), R, Ccols,
                       D, col_offset, n_local, (float)inv_temp, (float)gscale, optf32(gout, "gout"),
                       f32w(part, "part"), splits, f32w(out, "out"), cur_stream());
}
void nt_normalize_backward(const Tensor& zn, const Tensor& inv_norm, const Tensor& dzn,
                           const c10::optional<Tensor>& dz_bf16, const c10::optional<Tensor>& dz_f32) {
  const int R = zn.size(0), D = zn.size(1);
  TORCH_CHECK(dzn.numel() == (int64_t)R * D, "nt_normalize_backward sizes");
  ntxent_normalize_backward(f32(zn, "zn"), f32(inv_norm, "inv_norm"), f32(dzn, "dzn"), R, D,
                            optbfw(dz_bf16, "dz_bf16"), optf32w(dz_f32, "dz_f32"), cur_stream());
}
void nt_reduce_loss(const Tensor& loss_rows, double scale, const Tensor& out) {
  ntxent_reduce_loss(f32(loss_rows, "loss_rows"), loss_rows.numel(), (float)scale, f32w(out, "out"),
                     cur_stream());
}
// ---- weighted negatives (loss.hard_beta / loss.tau_plus / loss.decoupled): part holds 5 floats
// per row and split if hard_beta > 0, else 3; stats [R][4] = (L1, A, B, L0) per row
void check_nt_weighted(const char* op, double hard_beta, double tau_plus) {
  TORCH_CHECK(std::isfinite(hard_beta) && hard_beta >= 0.0, op,
              ": hard_beta must be a finite number >= 0, got ", hard_beta);
  TORCH_CHECK(std::isfinite(tau_plus) && tau_plus >= 0.0 && tau_plus < 1.0, op,
              ": tau_plus must be in [0, 1), got ", tau_plus);
}
void nt_w_forward_range(const Tensor& znT, int64_t R, int64_t col_offset, int64_t n_local,
                        double inv_temp, double hard_beta, const Tensor& part, int64_t c_lo,
                        int64_t c_hi, int64_t splits, int64_t split_base) {
  TORCH_CHECK(znT.dim() == 2, "nt_w_forward_range: znT must be [D][Ccols]");
  const int D = znT.size(0), Ccols = znT.size(1);
  check_nt(R, Ccols, D, col_offset, n_local);
  check_nt_weighted("nt_w_forward_range", hard_beta, 0.0);
  const int64_t np = hard_beta > 0.0 ? 5 : 3;
  TORCH_CHECK(c_lo >= 0 && c_lo < c_hi && c_hi <= Ccols && c_lo % 16 == 0 && c_hi % 16 == 0 &&
                  splits >= 1 && split_base >= 0,
              "nt_w_forward_range: column window / splits");
  TORCH_CHECK(part.numel() >= (split_base + splits) * R * np,
              "nt_w_forward_range: part must hold (split_base + splits) * R * ", np, " floats, got ",
              part.numel());
  ntxent_weighted_forward_range(f32(znT, "znT"), R, Ccols, D, col_offset, n_local, (float)inv_temp,
                                (float)hard_beta, f32w(part, "part"), c_lo, c_hi, splits,
                                split_base, cur_stream());
}
void nt_w_finish(const Tensor& part, int64_t R, int64_t splits, int64_t Ccols, double inv_temp,
                 double hard_beta, double tau_plus, bool decoupled, const Tensor& stats,
                 const Tensor& loss) {
  check_nt_weighted("nt_w_finish", hard_beta, tau_plus);
  const int64_t np = hard_beta > 0.0 ? 5 : 3;
  TORCH_CHECK(R >= 1 && splits >= 1 && Ccols >= R && Ccols % 16 == 0 && Ccols < (1LL << 24),
              "nt_w_finish: R / splits / Ccols");
  TORCH_CHECK(part.numel() >= splits * R * np, "nt_w_finish: part must hold splits * R * ", np,
              " floats, got ", part.numel());
  TORCH_CHECK(stats.numel() == R * 4, "nt_w_finish: stats must hold R * 4 floats, got ",
              stats.numel());
  TORCH_CHECK(((uintptr_t)stats.data_ptr() & 15) == 0, "nt_w_finish: stats must be 16-byte aligned");
  TORCH_CHECK(loss.numel() == R, "nt_w_finish: loss must hold R floats, got ", loss.numel());
  ntxent_weighted_finish(f32(part, "part"), R, splits, Ccols, (float)inv_temp, (float)hard_beta,
                         (float)tau_plus, decoupled ? 1 : 0, f32w(stats, "stats"),
                         f32w(loss, "loss"), cur_stream());
}
void nt_w_backward_part(bool row_mode, const Tensor& zn, const Tensor& znT, const Tensor& stats,
                        int64_t R, int64_t col_offset, int64_t n_local, double inv_temp,
                        double hard_beta, double gscale, const c10::optional<Tensor>& gout,
                        const Tensor& part, int64_t splits, const Tensor& out) {
  TORCH_CHECK(znT.dim() == 2, "nt_w_backward: znT must be [D][Ccols]");
  const int D = znT.size(0), Ccols = znT.size(1);
  check_nt(R, Ccols, D, col_offset, n_local);
  check_nt_weighted("nt_w_backward", hard_beta, 0.0);
  TORCH_CHECK(zn.numel() == (int64_t)Ccols * D, "nt_w_backward: zn size");
  TORCH_CHECK(stats.numel() == R * 4, "nt_w_backward: stats must hold R * 4 floats, got ",
              stats.numel());
  TORCH_CHECK(((uintptr_t)stats.data_ptr() & 15) == 0,
              "nt_w_backward: stats must be 16-byte aligned");
  const int64_t nown = row_mode ? R : Ccols;
  TORCH_CHECK(splits >= 1 && part.numel() >= splits * nown * D && out.numel() == nown * D,
              "nt_w_backward sizes");
  ntxent_weighted_backward_part(row_mode ? 1 : 0, f32(zn, "zn"), f32(znT, "znT"),
                                f32(stats, "stats"), R, Ccols, D, col_offset, n_local,
                                (float)inv_temp, (float)hard_beta, (float)gscale,
                                optf32(gout, "gout"), f32w(part, "part"), splits, f32w(out, "out"),
                                cur_stream());
}
// ---- label mode (SupCon): ycol = the columns' int32 labels
// ycol covers the columns [y0, y0 + len): the scored window and the rank's own rows lie inside
void nt_sup_forward_range(const Tensor& znT, const Tensor& ycol, int64_t y0, int64_t R,
                          int64_t col_offset, int64_t n_local, double inv_temp, const Tensor& part,
                          int64_t c_lo, int64_t c_hi, int64_t splits, int64_t split_base) {
  const int D = znT.size(0), Ccols = znT.size(1);
  check_nt(R, Ccols, D, col_offset, n_local);
  TORCH_CHECK(c_lo >= 0 && c_lo < c_hi && c_hi <= Ccols && c_lo % 16 == 0 && c_hi % 16 == 0 &&
                  splits >= 1 && split_base >= 0 && part.numel() >= (split_base + splits) * R * 4,
              "nt_sup_forward_range: column window / splits");
  const int* y = i32(ycol, "nt_sup_forward_range: ycol");
  const int64_t y1 = y0 + ycol.numel();
  TORCH_CHECK(y0 >= 0 && y0 % 16 == 0 && y1 <= Ccols && y0 <= c_lo && c_hi <= y1 &&
                  y0 <= col_offset && col_offset + R <= y1,
              "nt_sup_forward_range: ycol holds the labels of columns [", y0, ", ", y1,
              "), which must cover the window [", c_lo, ", ", c_hi, ") and the rows' own columns [",
              col_offset, ", ", col_offset + R, ")");
  supcon_forward_range(f32(znT, "znT"), y, y0, R, Ccols, D, col_offset, (float)inv_temp,
                       f32w(part, "part"), c_lo, c_hi, splits, split_base, cur_stream());
}
void nt_sup_finish(const Tensor& part, int64_t R, int64_t splits, const Tensor& lse,
                   const Tensor& inv_cnt, const Tensor& loss) {
  TORCH_CHECK(part.numel() >= splits * R * 4 && lse.numel() == R && inv_cnt.numel() == R &&
                  loss.numel() == R, "nt_sup_finish sizes");
  supcon_finish(f32(part, "part"), R, splits, f32w(lse, "lse"), f32w(inv_cnt, "inv_cnt"),
                f32w(loss, "loss"), cur_stream());
}
void nt_sup_backward_part(bool row_mode, const Tensor& zn, const Tensor& znT, const Tensor& lse,
                          const Tensor& inv_cnt, const Tensor& ycol, int64_t R, int64_t col_offset,
                          int64_t n_local, double inv_temp, double gscale,
                          const c10::optional<Tensor>& gout, const Tensor& part, int64_t splits,
                          const Tensor& out) {
  const int D = znT.size(0), Ccols = znT.size(1);
  check_nt(R, Ccols, D, col_offset, n_local);
  TORCH_CHECK(zn.numel() == (int64_t)Ccols * D, "nt_sup_backward: zn size");
  TORCH_CHECK(lse.numel() == R && inv_cnt.numel() == R, "nt_sup_backward: lse / inv_cnt size");
  const int* y = i32(ycol, "nt_sup_backward: ycol");
  TORCH_CHECK(ycol.numel() == Ccols, "nt_sup_backward: ycol must hold one label per column (",
              Ccols, "), got ", ycol.numel());
  const int64_t nown = row_mode ? R : Ccols;
  TORCH_CHECK(splits >= 1 && part.numel() >= splits * nown * D && out.numel() == nown * D,
              "nt_sup_backward sizes");
  supcon_backward_part(row_mode ? 1 : 0, f32(zn, "zn"), f32(znT, "znT"), f32(lse, "lse"),
                       f32(inv_cnt, "inv_cnt"), y, R, Ccols, D, col_offset, (float)inv_temp,
                       (float)gscale, optf32(gout, "gout"), f32w(part, "part"), splits,
                       f32w(out, "out"), cur_stream());
}
// out [views * n] int32 = labels[idx] (or labels itself, n of them) repeated once per view
void nt_expand_labels(const Tensor& labels, const c10::optional<Tensor>& idx, int64_t views,
                      const Tensor& out) {
  TORCH_CHECK(labels.is_cuda() && labels.is_contiguous() && labels.dim() == 1 &&
                  (labels.scalar_type() == at::kInt || labels.scalar_type() == at::kLong),
              "nt_expand_labels: labels must be a contiguous 1-D int32 or int64 GPU tensor, got ",
              labels.scalar_type());
  const bool has_idx = idx.has_value() && idx->defined();
  if (has_idx) check_dev(*idx, at::kLong, "nt_expand_labels: idx");
  const int64_t n = has_idx ? idx->numel() : labels.numel();
  TORCH_CHECK(views >= 1 && n >= 1 && labels.numel() >= 1 && views * n < (1LL << 31),
              "nt_expand_labels: empty input");
  check_dev(out, at::kInt, "nt_expand_labels: out");
  TORCH_CHECK(out.numel() == views * n, "nt_expand_labels: out must hold views * n = ", views * n,
              " labels, got ", out.numel());
  supcon_expand_labels(labels.data_ptr(), labels.scalar_type() == at::kLong ? 1 : 0,
                       has_idx ? idx->data_ptr<int64_t>() : nullptr, labels.numel(), (int)n,
                       (int)views, out.data_ptr<int>(), cur_stream());
}

// ------------------------------------------------------------------------------- nnclr
// (csrc/nnclr.hip; every tensor's size is checked against n, D and Q before any launch)
void check_nc(int64_t n, int64_t D, const char* what) {
  TORCH_CHECK(n >= 16 && n % 16 == 0 && n <= (1 << 20), what, ": n must be a multiple of 16 in "
              "[16, 2^20], got ", n);
  TORCH_CHECK(D == 32 || D == 64 || D == 128 || D == 256, what, ": D must be 32, 64, 128 or 256, "
              "got ", D);
}
void check_nc_queue(const Tensor& queue, int64_t n, int64_t D, const char* what) {
  TORCH_CHECK(queue.dim() == 2 && queue.size(1) == D, what, ": the queue must be [Q][", D,
              "], got ", queue.sizes());
  const int64_t Q = queue.size(0);
  TORCH_CHECK(Q >= 256 && Q % 256 == 0 && Q <= (1 << 20) && n <= Q, what, ": Q must be a "
              "multiple of 256 in [256, 2^20] and at least n = ", n, ", got ", Q);
}
// [2n][D] of the given dtype
void check_nc_rows(const Tensor& t, int64_t n, int64_t D, const char* what, const char* name) {
  TORCH_CHECK(t.dim() == 2 && t.size(0) == 2 * n && t.size(1) == D, what, ": ", name,
              " must be [", 2 * n, "][", D, "], got ", t.sizes());
}
int64_t nc_top1_splits(int64_t R, int64_t Q) {
  TORCH_CHECK(R >= 32 && R % 32 == 0 && Q >= 256 && Q % 256 == 0 && Q <= (1 << 20),
              "nc_top1_splits: R must be a multiple of 32 and Q a multiple of 256, got R ", R,
              ", Q ", Q);
  return nnclr_top1_splits((int)R, (int)Q);
}
int64_t nc_loss_splits(int64_t n) {
  check_nc(n, 32, "nc_loss_splits");
  return nnclr_loss_splits((int)n);
}
void nc_normalize(const Tensor& z, const Tensor& zn, const Tensor& zb, const Tensor& inv_norm) {
  TORCH_CHECK(z.dim() == 2 && z.size(0) % 2 == 0, "nc_normalize: z must be [2n][D]");
  const int64_t n = z.size(0) / 2, D = z.size(1);
  check_nc(n, D, "nc_normalize");
  TORCH_CHECK(z.is_cuda() && z.is_contiguous() &&
                  (z.scalar_type() == at::kBFloat16 || z.scalar_type() == at::kFloat),
              "nc_normalize: z must be a contiguous bf16 or fp32 GPU tensor");
  check_nc_rows(zn, n, D, "nc_normalize", "zn");
  check_nc_rows(zb, n, D, "nc_normalize", "zb");
  TORCH_CHECK(inv_norm.numel() == 2 * n, "nc_normalize: inv_norm must hold 2n = ", 2 * n,
              " values, got ", inv_norm.numel());
  nnclr_normalize(z.data_ptr(), z.scalar_type() == at::kFloat ? 1 : 0, (int)(2 * n), (int)D,
                  f32w(zn, "zn"), bfw(zb, "zb"), f32w(inv_norm, "inv_norm"), cur_stream());
}
void nc_lookup(const Tensor& zb, const Tensor& queue, int64_t splits, const Tensor& candv,
               const Tensor& candi, const Tensor& idx, const Tensor& a) {
  TORCH_CHECK(zb.dim() == 2 && zb.size(0) % 2 == 0, "nc_lookup: zb must be [2n][D]");
  const int64_t n = zb.size(0) / 2, D = zb.size(1), R = 2 * n;
  check_nc(n, D, "nc_lookup");
  check_nc_queue(queue, n, D, "nc_lookup");
  const int64_t Q = queue.size(0);
  TORCH_CHECK(splits >= 1 && splits <= Q / 64, "nc_lookup: 1 <= splits <= Q / 64, got ", splits);
  TORCH_CHECK(candv.numel() == splits * R && candi.numel() == splits * R,
              "nc_lookup: candv / candi must be [splits][2n] = ", splits * R, " values, got ",
              candv.numel(), " / ", candi.numel());
  TORCH_CHECK(idx.numel() == R, "nc_lookup: idx must hold 2n = ", R, " values, got ", idx.numel());
  check_nc_rows(a, n, D, "nc_lookup", "a");
  check_dev(candi, at::kInt, "nc_lookup: candi");
  check_dev(idx, at::kInt, "nc_lookup: idx");
  nnclr_lookup(bf(zb, "zb"), bf(queue, "queue"), (int)R, (int)Q, (int)D, (int)splits,
               f32w(candv, "candv"), candi.data_ptr<int>(), idx.data_ptr<int>(), bfw(a, "a"),
               cur_stream());
}
void nc_forward(const Tensor& a, const Tensor& zb, double inv_temp, int64_t splits,
                const Tensor& part) {
  TORCH_CHECK(zb.dim() == 2 && zb.size(0) % 2 == 0, "nc_forward: zb must be [2n][D]");
  const int64_t n = zb.size(0) / 2, D = zb.size(1);
  check_nc(n, D, "nc_forward");
  check_nc_rows(a, n, D, "nc_forward", "a");
  TORCH_CHECK(splits >= 1 && splits <= n / 16 && part.numel() == splits * 2 * n * 3,
              "nc_forward: part must be [splits][2n][3] with 1 <= splits <= n / 16, got splits ",
              splits, ", ", part.numel(), " values");
  TORCH_CHECK(inv_temp > 0.0, "nc_forward: the temperature must be > 0");
  nnclr_forward(bf(a, "a"), bf(zb, "zb"), (int)n, (int)D, (float)inv_temp, (int)splits,
                f32w(part, "part"), cur_stream());
}
void nc_backward(const Tensor& a, const Tensor& zb, const Tensor& zn, const Tensor& inv_norm,
                 const Tensor& lse, double inv_temp, const Tensor& gout, int64_t splits,
                 const Tensor& part, const c10::optional<Tensor>& dz_bf16,
                 const c10::optional<Tensor>& dz_f32) {
  TORCH_CHECK(zb.dim() == 2 && zb.size(0) % 2 == 0, "nc_backward: zb must be [2n][D]");
  const int64_t n = zb.size(0) / 2, D = zb.size(1);
  check_nc(n, D, "nc_backward");
  check_nc_rows(a, n, D, "nc_backward", "a");
  check_nc_rows(zn, n, D, "nc_backward", "zn");
  TORCH_CHECK(inv_norm.numel() == 2 * n && lse.numel() == 2 * n && gout.numel() == 1,
              "nc_backward: inv_norm and lse must hold 2n = ", 2 * n, " values and gout one");
  TORCH_CHECK(splits >= 1 && splits <= n / 16 && part.numel() == splits * 2 * n * D,
              "nc_backward: part must be [splits][2n][D] with 1 <= splits <= n / 16, got splits ",
              splits, ", ", part.numel(), " values");
  uint16_t* ob = optbfw(dz_bf16, "dz_bf16");
  float* of = optf32w(dz_f32, "dz_f32");
  TORCH_CHECK((ob != nullptr) != (of != nullptr), "nc_backward: one of dz_bf16 / dz_f32");
  TORCH_CHECK((ob ? dz_bf16->numel() : dz_f32->numel()) == 2 * n * D, "nc_backward: dz size");
  nnclr_backward(bf(a, "a"), bf(zb, "zb"), f32(zn, "zn"), f32(inv_norm, "inv_norm"),
                 f32(lse, "lse"), (int)n, (int)D, (float)inv_temp, f32(gout, "gout"), (int)splits,
                 f32w(part, "part"), ob, of, cur_stream());
}
void nc_enqueue(const Tensor& zb, const Tensor& queue, const Tensor& cursor) {
  TORCH_CHECK(zb.dim() == 2 && zb.size(0) % 2 == 0, "nc_enqueue: zb must be [2n][D]");
  const int64_t n = zb.size(0) / 2, D = zb.size(1);
  check_nc(n, D, "nc_enqueue");
  check_nc_queue(queue, n, D, "nc_enqueue");
  check_dev(cursor, at::kInt, "nc_enqueue: cursor");
  TORCH_CHECK(cursor.numel() == 1, "nc_enqueue: the cursor is one int32");
  nnclr_enqueue(bf(zb, "zb"), (int)n, (int)D, (int)queue.size(0), bfw(queue, "queue"),
                cursor.data_ptr<int>(), cur_stream());
}

// ------------------------------------------------------------------------------- barlow twins
// (csrc/barlow.hip; every tensor's size is checked against n and D before any launch)
void check_bt(int64_t n, int64_t D) {
  TORCH_CHECK(n >= 32 && n % 32 == 0 && n <= (1 << 20), "barlow: n must be a multiple of 32 in "
              "[32, 2^20], got ", n);
  TORCH_CHECK(D >= 64 && D <= 2048 && D % 64 == 0, "barlow: D must be a multiple of 64 in "
              "[64, 2048], got ", D);
}
void check_bt_z(const Tensor& z, const char* what) {
  TORCH_CHECK(z.dim() == 2 && z.size(0) % 2 == 0, what, ": z must be [2n][D]");
  check_bt(z.size(0) / 2, z.size(1));
  TORCH_CHECK(z.is_cuda() && z.is_contiguous() &&
                  (z.scalar_type() == at::kBFloat16 || z.scalar_type() == at::kFloat),
              what, ": z must be a contiguous bf16 or fp32 GPU tensor");
}
// (bf() checks the dtype, the device and the layout where the pointer is taken)
void check_bt_zh(const Tensor& zh, const char* what) {
  TORCH_CHECK(zh.dim() == 2 && zh.size(0) % 2 == 0, what, ": zh must be [2n][D]");
  check_bt(zh.size(0) / 2, zh.size(1));
}
// exactly one of dz_bf16 / dz_f32, of `numel` elements -> (bf16, fp32) pointers, one of them null
std::pair<uint16_t*, float*> bt_dz(const c10::optional<Tensor>& dz_bf16,
                                   const c10::optional<Tensor>& dz_f32, int64_t numel,
                                   const char* what) {
  uint16_t* ob = optbfw(dz_bf16, "dz_bf16");
  float* of = optf32w(dz_f32, "dz_f32");
  TORCH_CHECK((ob != nullptr) != (of != nullptr), what, ": one of dz_bf16 / dz_f32");
  TORCH_CHECK((ob ? dz_bf16->numel() : dz_f32->numel()) == numel, what, ": dz size");
  return {ob, of};
}
void bt_standardize(const Tensor& z, double eps, const Tensor& rstd, const Tensor& zh,
                    const Tensor& zhT) {
  check_bt_z(z, "bt_standardize");
  const int64_t n = z.size(0) / 2, D = z.size(1);
  TORCH_CHECK(eps > 0.0, "bt_standardize: eps must be > 0");
  TORCH_CHECK(rstd.numel() == 2 * D && zh.numel() == 2 * n * D && zhT.numel() == 2 * n * D,
              "bt_standardize sizes");
  barlow_standardize(z.data_ptr(), z.scalar_type() == at::kFloat ? 1 : 0, (int)n, (int)D,
                     (float)eps, f32w(rstd, "rstd"), bfw(zh, "zh"), bfw(zhT, "zhT"), cur_stream());
}
int64_t bt_corr_splits(int64_t n, int64_t D) {
  check_bt(n, D);
  return barlow_corr_splits((int)n, (int)D);
}
int64_t bt_loss_blocks(int64_t D) {
  check_bt(32, D);
  return barlow_loss_blocks((int)D);
}
void bt_corr(const Tensor& zhT, int64_t n, int64_t splits, const Tensor& part) {
  TORCH_CHECK(zhT.dim() == 3 && zhT.size(0) == 2 && zhT.size(2) == n, "bt_corr: zhT is [2][D][n]");
  const int64_t D = zhT.size(1);
  check_bt(n, D);
  TORCH_CHECK(splits >= 1 && splits <= n / 32 && part.numel() == splits * D * D,
              "bt_corr: part must be [splits][D][D] with 1 <= splits <= n / 32");
  barlow_corr(bf(zhT, "zhT"), (int)n, (int)D, (int)splits, f32w(part, "part"), cur_stream());
}
void bt_loss(const Tensor& part, int64_t splits, int64_t n, double lambd, const Tensor& C,
             const Tensor& lpart) {
  TORCH_CHECK(C.dim() == 2 && C.size(0) == C.size(1), "bt_loss: C is [D][D]");
  const int64_t D = C.size(0);
  check_bt(n, D);
  TORCH_CHECK(splits >= 1 && part.numel() == splits * D * D &&
                  lpart.numel() == barlow_loss_blocks((int)D), "bt_loss sizes");
  barlow_loss(f32(part, "part"), (int)splits, (int)n, (int)D, (float)lambd, f32w(C, "C"),
              f32w(lpart, "lpart"), cur_stream());
}
void bt_grad(const Tensor& C, double lambd, const Tensor& gout, const Tensor& G,
             const Tensor& GT) {
  TORCH_CHECK(C.dim() == 2 && C.size(0) == C.size(1), "bt_grad: C is [D][D]");
  const int64_t D = C.size(0);
  check_bt(32, D);
  TORCH_CHECK(gout.numel() == 1 && G.numel() == D * D && GT.numel() == D * D, "bt_grad sizes");
  barlow_grad(f32(C, "C"), (int)D, (float)lambd, f32(gout, "gout"), bfw(G, "G"), bfw(GT, "GT"),
              cur_stream());
}
void bt_backward(const Tensor& zh, const Tensor& G, const Tensor& GT, const Tensor& dzh,
                 const Tensor& colpart) {
  check_bt_zh(zh, "bt_backward");
  const int64_t n = zh.size(0) / 2, D = zh.size(1);
  TORCH_CHECK(G.numel() == D * D && GT.numel() == D * D && dzh.numel() == 2 * n * D &&
                  colpart.numel() == 2 * (n / 32) * 2 * D, "bt_backward sizes");
  barlow_backward(bf(zh, "zh"), bf(G, "G"), bf(GT, "GT"), (int)n, (int)D, f32w(dzh, "dzh"),
                  f32w(colpart, "colpart"), cur_stream());
}
void bt_std_backward(const Tensor& zh, const Tensor& rstd, const Tensor& dzh,
                     const Tensor& colpart, const c10::optional<Tensor>& dz_bf16,
                     const c10::optional<Tensor>& dz_f32) {
  check_bt_zh(zh, "bt_std_backward");
  const int64_t n = zh.size(0) / 2, D = zh.size(1);
  TORCH_CHECK(rstd.numel() == 2 * D && dzh.numel() == 2 * n * D &&
                  colpart.numel() == 2 * (n / 32) * 2 * D, "bt_std_backward sizes");
  const auto dz = bt_dz(dz_bf16, dz_f32, 2 * n * D, "bt_std_backward");
  barlow_std_backward(bf(zh, "zh"), f32(rstd, "rstd"), f32(dzh, "dzh"), f32(colpart, "colpart"),
                      (int)n, (int)D, dz.first, dz.second, cur_stream());
}
// the loss over W ranks (loss.barlow_global): W is the leading size of the gathered tensors,
// g = gstats or gsum [W][2][2][D] -> W
int64_t check_bt_gathered(const Tensor& g, int64_t n, int64_t D, const char* what,
                          const char* name) {
  TORCH_CHECK(g.dim() == 4 && g.size(1) == 2 && g.size(2) == 2 && g.size(3) == D, what, ": ", name,
              " must be [W][2][2][D] with D = ", D);
  const int64_t W = g.size(0);
  TORCH_CHECK(W >= 1 && W <= 1024 && W * n <= (1 << 20), what, ": W ranks of n rows need "
              "1 <= W <= 1024 and W * n <= 2^20, got W ", W, ", n ", n);
  return W;
}
void bt_stats(const Tensor& z, const Tensor& stats) {
  check_bt_z(z, "bt_stats");
  const int64_t n = z.size(0) / 2, D = z.size(1);
  TORCH_CHECK(stats.numel() == 4 * D, "bt_stats: stats must be [2][2][D] = ", 4 * D,
              " values, got ", stats.numel());
  barlow_stats(z.data_ptr(), z.scalar_type() == at::kFloat ? 1 : 0, (int)n, (int)D,
               f32w(stats, "stats"), cur_stream());
}
void bt_merge_standardize(const Tensor& z, const Tensor& gstats, double eps, const Tensor& rstd,
                          const Tensor& zh, const Tensor& zhT) {
  check_bt_z(z, "bt_merge_standardize");
  const int64_t n = z.size(0) / 2, D = z.size(1);
  const int64_t W = check_bt_gathered(gstats, n, D, "bt_merge_standardize", "gstats");
  TORCH_CHECK(eps > 0.0, "bt_merge_standardize: eps must be > 0");
  TORCH_CHECK(rstd.numel() == 2 * D && zh.numel() == 2 * n * D && zhT.numel() == 2 * n * D,
              "bt_merge_standardize sizes: rstd [2][D], zh [2n][D], zhT [2][D][n]");
  barlow_merge_standardize(z.data_ptr(), z.scalar_type() == at::kFloat ? 1 : 0,
                           f32(gstats, "gstats"), (int)W, (int)n, (int)D, (float)eps,
                           f32w(rstd, "rstd"), bfw(zh, "zh"), bfw(zhT, "zhT"), cur_stream());
}
void bt_slab_merge(const Tensor& part, int64_t splits, const Tensor& S) {
  TORCH_CHECK(S.dim() == 2 && S.size(0) == S.size(1), "bt_slab_merge: S is [D][D]");
  const int64_t D = S.size(0);
  check_bt(32, D);
  TORCH_CHECK(splits >= 1 && part.numel() == splits * D * D,
              "bt_slab_merge: part must be [splits][D][D]");
  barlow_slab_merge(f32(part, "part"), (int)splits, (int)D, f32w(S, "S"), cur_stream());
}
void bt_colsum(const Tensor& colpart, const Tensor& csum) {
  TORCH_CHECK(colpart.dim() == 4 && colpart.size(0) == 2 && colpart.size(2) == 2,
              "bt_colsum: colpart must be [2][n/32][2][D]");
  const int64_t n = colpart.size(1) * 32, D = colpart.size(3);
  check_bt(n, D);
  TORCH_CHECK(csum.numel() == 4 * D, "bt_colsum: csum must be [2][2][D] = ", 4 * D,
              " values, got ", csum.numel());
  barlow_colsum(f32(colpart, "colpart"), (int)n, (int)D, f32w(csum, "csum"), cur_stream());
}
void bt_std_backward_global(const Tensor& zh, const Tensor& rstd, const Tensor& dzh,
                            const Tensor& gsum, const c10::optional<Tensor>& dz_bf16,
                            const c10::optional<Tensor>& dz_f32) {
  check_bt_zh(zh, "bt_std_backward_global");
  const int64_t n = zh.size(0) / 2, D = zh.size(1);
  const int64_t W = check_bt_gathered(gsum, n, D, "bt_std_backward_global", "gsum");
  TORCH_CHECK(rstd.numel() == 2 * D && dzh.numel() == 2 * n * D,
              "bt_std_backward_global sizes: rstd [2][D], dzh [2n][D]");
  const auto dz = bt_dz(dz_bf16, dz_f32, 2 * n * D, "bt_std_backward_global");
  barlow_std_backward_global(bf(zh, "zh"), f32(rstd, "rstd"), f32(dzh, "dzh"), f32(gsum, "gsum"),
                             (int)W, (int)n, (int)D, dz.first, dz.second, cur_stream());
}

// ------------------------------------------------------------------------------- lars
void lars_norms_op(const Tensor& p, const Tensor& g, const Tensor& chunk_beg,
                   const Tensor& chunk_end, double grad_scale, const Tensor& norms) {
  const int nchunks = chunk_beg.numel();
  TORCH_CHECK(norms.numel() >= 2 * nchunks && p.numel() == g.numel(), "lars_norms sizes");
  lars_norms(f32(p, "p"), f32(g, "g"), i32(chunk_beg, "chunk_beg"), i32(chunk_end, "chunk_end"),
             nchunks, (float)grad_scale, f32w(norms, "norms"), cur_stream());
}
void lars_update_op(const Tensor& p, const Tensor& g, const Tensor& mom,
                    const c10::optional<Tensor>& shadow, const Tensor& chunk_seg,
                    const Tensor& chunk_beg, const Tensor& chunk_end, const Tensor& seg_chunk_beg,
                    const Tensor& seg_chunk_end, const Tensor& seg_wd, const Tensor& seg_flags,
                    const Tensor& norms, const Tensor& lr, double momentum, double trust, double eps,
                    double grad_scale, bool nesterov) {
  const int nchunks = chunk_beg.numel();
  TORCH_CHECK(p.numel() == g.numel() && p.numel() == mom.numel(), "lars_update sizes");
  if (shadow.has_value() && shadow->defined())
    TORCH_CHECK(shadow->numel() == p.numel(), "lars_update: shadow size");
  lars_update(f32w(p, "p"), f32(g, "g"), f32w(mom, "mom"), optbfw(shadow, "shadow"),
              i32(chunk_seg, "chunk_seg"), i32(chunk_beg, "chunk_beg"), i32(chunk_end, "chunk_end"),
              nchunks, i32(seg_chunk_beg, "seg_chunk_beg"), i32(seg_chunk_end, "seg_chunk_end"),
              f32(seg_wd, "seg_wd"), i32(seg_flags, "seg_flags"), f32(norms, "norms"),
              f32(lr, "lr"), (float)momentum, (float)trust, (float)eps, (float)grad_scale,
              nesterov ? 1 : 0, cur_stream());
}
void lr_step_op(const Tensor& step, const Tensor& lr, double lr0, int64_t warmup, int64_t total,
                int64_t mode) {
  check_dev(step, at::kLong, "step");
  lr_schedule_step(step.data_ptr<int64_t>(), f32w(lr, "lr"), lr0, warmup, total, (int)mode,
                   cur_stream());
}

// ------------------------------------------------------------------------------- augment
void augment_op(const Tensor& images, const c10::optional<Tensor>& indices, int64_t n,
                int64_t views, int64_t OH, int64_t OW, int64_t Cpad, double strength, int64_t seed,
                int64_t counter, int64_t view_offset, int64_t flags, const Tensor& out,
                const c10::optional<Tensor>& params, int64_t blur_kernel) {
  check_dev(images, at::kByte, "images");
  TORCH_CHECK(n >= 0 && views >= 0 && OH > 0 && OW > 0, "augment: sizes");
  if (blur_kernel != 0) {
    // Gaussian blur (augment.hip): an odd kernel in [3, limit] whose half width reflect padding
    // can serve, on augmented launches only, at a size whose bands fit the kernel's LDS
    const int64_t lim = augment_max_blur_kernel();
    TORCH_CHECK(blur_kernel >= 3 && blur_kernel % 2 == 1 && blur_kernel <= lim,
                "augment: blur_kernel must be 0 (off) or odd in [3, ", lim, "], got ", blur_kernel);
    TORCH_CHECK((blur_kernel - 1) / 2 <= std::min(OH, OW) - 1, "augment: blur_kernel ",
                blur_kernel, " too large for reflect padding of a ", OH, "x", OW, " output");
    TORCH_CHECK(flags & 1, "augment: blur_kernel needs the augmented mode (flags & 1)");
    TORCH_CHECK(augment_blur_band((int)OH, (int)OW, (int)blur_kernel) > 0, "augment: a ", OH, "x",
                OW, " output with blur_kernel ", blur_kernel, " does not fit the blur's LDS bands");
  }
  TORCH_CHECK(images.dim() == 4 && images.size(3) == 3, "augment: images must be [N,H,W,3] uint8");
  const int H = images.size(1), W = images.size(2);
  TORCH_CHECK(Cpad >= 3, "augment: Cpad >= 3");
  TORCH_CHECK(out.numel() == views * n * OH * OW * Cpad, "augment: out size");
  const int64_t* idx = nullptr;
  if (indices.has_value() && indices->defined()) {
    check_dev(*indices, at::kLong, "indices");
    TORCH_CHECK(indices->numel() >= n, "augment: indices size");
    idx = indices->data_ptr<int64_t>();
  } else {
    TORCH_CHECK(n <= images.size(0), "augment: n > dataset");
  }
  if (!(flags & 1)) TORCH_CHECK(OH == H && OW == W, "augment: plain mode needs OH==H, OW==W");
  float* po = nullptr;
  if (params.has_value() && params->defined()) {
    TORCH_CHECK(params->numel() >= views * n * 16, "augment: params size");
    po = f32w(*params, "params");
  }
  simclr_augment(images.data_ptr<uint8_t>(), idx, n, views, H, W, OH, OW, Cpad, (float)strength,
                 (uint64_t)seed, (uint64_t)counter, view_offset, flags, bfw(out, "out"), po,
                 (int)blur_kernel, cur_stream());
}

int64_t augment_max_blur_kernel_op() { return augment_max_blur_kernel(); }

// ---- eval.hip: maxpool (K2), cross-entropy + top-k (K10), centroid class sums (K11)
void maxpool_fwd_op(const Tensor& x, const Tensor& y, const Tensor& arg, int64_t K, int64_t S,
                    int64_t P) {
  TORCH_CHECK(x.dim() == 4 && y.dim() == 4, "maxpool: NHWC 4-D tensors expected");
  const int Nb = x.size(0), H = x.size(1), W = x.size(2), C = x.size(3);
  const int OH = (H + 2 * P - K) / S + 1, OW = (W + 2 * P - K) / S + 1;
  TORCH_CHECK(C % 8 == 0 && K >= 1 && K * K <= 255 && S >= 1 && P >= 0 && P < K,
              "maxpool: C % 8 == 0, K*K <= 255, 0 <= P < K");
  TORCH_CHECK(y.size(0) == Nb && y.size(1) == OH && y.size(2) == OW && y.size(3) == C,
              "maxpool: output shape");
  check_dev(arg, at::kByte, "arg");
  TORCH_CHECK(arg.numel() == y.numel(), "maxpool: argmax size");
  maxpool_fwd(bf(x, "x"), bfw(y, "y"), arg.data_ptr<uint8_t>(), Nb, H, W, C, OH, OW, (int)K,
              (int)S, (int)P, cur_stream());
}

void maxpool_bwd_op(const Tensor& dy, const Tensor& arg, const Tensor& dx, int64_t K, int64_t S,
                    int64_t P) {
  TORCH_CHECK(dy.dim() == 4 && dx.dim() == 4, "maxpool_bwd: NHWC 4-D tensors expected");
  const int Nb = dx.size(0), H = dx.size(1), W = dx.size(2), C = dx.size(3);
  const int OH = (H + 2 * P - K) / S + 1, OW = (W + 2 * P - K) / S + 1;
  TORCH_CHECK(C % 8 == 0 && K * K <= 255 && P < K, "maxpool_bwd: geometry");
  TORCH_CHECK(dy.size(0) == Nb && dy.size(1) == OH && dy.size(2) == OW && dy.size(3) == C,
              "maxpool_bwd: dy shape");
  check_dev(arg, at::kByte, "arg");
  TORCH_CHECK(arg.numel() == dy.numel(), "maxpool_bwd: argmax size");
  maxpool_bwd(bf(dy, "dy"), arg.data_ptr<uint8_t>(), bfw(dx, "dx"), Nb, H, W, C, OH, OW, (int)K,
              (int)S, (int)P, cur_stream());
}

// split-K small-M GEMM (projection head GEMM 2): out = relu(bn(A))·Bᵀ + bias
void gemm_sk_op(const Tensor& A, const Tensor& B, const c10::optional<Tensor>& sc,
                const c10::optional<Tensor>& sh, int64_t seg, int64_t KS, const Tensor& part,
                const c10::optional<Tensor>& bias, const Tensor& out) {
  TORCH_CHECK(A.dim() == 2 && B.dim() == 2 && out.dim() == 2, "gemm_sk: 2-D operands");
  const int64_t M = A.size(0), K = A.size(1), N = B.size(0);
  TORCH_CHECK(B.size(1) == K && out.size(0) == M && out.size(1) == N, "gemm_sk: shapes");
  TORCH_CHECK(M % 64 == 0 && N % 64 == 0 && KS >= 1 && K % (KS * 32) == 0 && K / KS <= 512,
              "gemm_sk: M, N multiples of 64; K / KS a multiple of 32, at most 512");
  TORCH_CHECK(part.numel() >= KS * M * N, "gemm_sk: partial scratch size");
  TORCH_CHECK(sc.has_value() == sh.has_value(), "gemm_sk: sc and sh together");
  if (sc.has_value()) {
    TORCH_CHECK(seg >= 1 && M % seg == 0, "gemm_sk: row segments");
    TORCH_CHECK(sc->numel() >= (M / seg) * K && sh->numel() >= (M / seg) * K,
                "gemm_sk: per-segment scale / shift tables");
  }
  if (bias.has_value()) TORCH_CHECK(bias->numel() == N, "gemm_sk: bias size");
  gemm_sk(bf(A, "A"), bf(B, "B"), sc.has_value() ? f32(*sc, "sc") : nullptr,
          sh.has_value() ? f32(*sh, "sh") : nullptr, (int)seg, (int)M, (int)N, (int)K, (int)KS,
          f32w(part, "part"), bias.has_value() ? f32(*bias, "bias") : nullptr, bfw(out, "out"),
          cur_stream());
}

// ImageNet stem: 2x2 space-to-depth of the zero-padded image (7x7/s2 -> 4x4/s1 conv)
void stem_s2d_op(const Tensor& img, int64_t creal, int64_t P, const Tensor& xs) {
  TORCH_CHECK(img.dim() == 4 && xs.dim() == 4, "stem_s2d: NHWC 4-D");
  const int Nb = img.size(0), H = img.size(1), W = img.size(2), Cin = img.size(3);
  TORCH_CHECK(Cin % 4 == 0 && creal >= 1 && creal <= 4 && P >= 0, "stem_s2d: channels / pad");
  TORCH_CHECK((H + 2 * P) % 2 == 0 && (W + 2 * P) % 2 == 0, "stem_s2d: padded size must be even");
  TORCH_CHECK(xs.size(0) == Nb && xs.size(1) == (H + 2 * P) / 2 && xs.size(2) == (W + 2 * P) / 2 &&
                  xs.size(3) == 16, "stem_s2d: output shape");
  stem_s2d(bf(img, "img"), bfw(xs, "xs"), Nb, H, W, Cin, (int)creal, (int)xs.size(1),
           (int)xs.size(2), (int)P, cur_stream());
}

// pooled ImageNet stem: BN + ReLU + max-pool forward, max-pool + ReLU-mask + BN backward
void bn_relu_maxpool_op(const Tensor& a, const Tensor& ss, int64_t S, const Tensor& y,
                        const Tensor& arg, const Tensor& asel, int64_t K, int64_t Sd, int64_t P) {
  TORCH_CHECK(a.dim() == 4 && y.dim() == 4 && asel.dim() == 4, "bn_relu_maxpool: NHWC 4-D");
  const int Nb = a.size(0), H = a.size(1), W = a.size(2), C = a.size(3);
  const int OH = (H + 2 * P - K) / Sd + 1, OW = (W + 2 * P - K) / Sd + 1;
  TORCH_CHECK(C % 8 == 0 && K >= 1 && K * K <= 255 && Sd >= 1 && P >= 0 && P < K,
              "bn_relu_maxpool: geometry");
  TORCH_CHECK(S >= 1 && Nb % S == 0, "bn_relu_maxpool: images must split evenly into views");
  TORCH_CHECK(y.size(0) == Nb && y.size(1) == OH && y.size(2) == OW && y.size(3) == C &&
                  asel.sizes() == y.sizes(), "bn_relu_maxpool: output shapes");
  TORCH_CHECK(ss.numel() == 2 * S * C, "bn_relu_maxpool: scale/shift table [2][S][C]");
  check_dev(arg, at::kByte, "arg");
  TORCH_CHECK(arg.numel() == y.numel(), "bn_relu_maxpool: argmax size");
  bn_relu_maxpool(bf(a, "a"), f32(ss, "ss"), (int)S, bfw(y, "y"), arg.data_ptr<uint8_t>(),
                  bfw(asel, "asel"), Nb, H, W, C, OH, OW, (int)K, (int)Sd, (int)P, cur_stream());
}

void maxpool_bwd_bn_op(const Tensor& gy, const Tensor& arg, const Tensor& y, const Tensor& a,
                       const Tensor& coef, int64_t S, const Tensor& da, int64_t K, int64_t Sd,
                       int64_t P) {
  TORCH_CHECK(a.dim() == 4 && da.dim() == 4 && gy.dim() == 4 && y.dim() == 4,
              "maxpool_bwd_bn: NHWC 4-D");
  const int Nb = a.size(0), H = a.size(1), W = a.size(2), C = a.size(3);
  const int OH = (H + 2 * P - K) / Sd + 1, OW = (W + 2 * P - K) / Sd + 1;
  TORCH_CHECK(C % 8 == 0 && K * K <= 255 && Sd >= 1 && P >= 0 && P < K, "maxpool_bwd_bn: geometry");
  TORCH_CHECK(S >= 1 && Nb % S == 0, "maxpool_bwd_bn: images must split evenly into views");
  TORCH_CHECK(gy.size(0) == Nb && gy.size(1) == OH && gy.size(2) == OW && gy.size(3) == C &&
                  y.sizes() == gy.sizes() && da.sizes() == a.sizes(),
              "maxpool_bwd_bn: shapes");
  TORCH_CHECK(coef.numel() == 3 * S * C, "maxpool_bwd_bn: coef [3][S][C]");
  check_dev(arg, at::kByte, "arg");
  TORCH_CHECK(arg.numel() == gy.numel(), "maxpool_bwd_bn: argmax size");
  maxpool_bwd_bn(bf(gy, "gy"), arg.data_ptr<uint8_t>(), bf(y, "y"), bf(a, "a"), f32(coef, "coef"),
                 (int)S, bfw(da, "da"), Nb, H, W, C, OH, OW, (int)K, (int)Sd, (int)P, cur_stream());
}

void ce_topk_op(const Tensor& logits, const Tensor& y, double gscale, const Tensor& loss,
                const Tensor& rank, const c10::optional<Tensor>& dlogits) {
  TORCH_CHECK(logits.dim() == 2, "ce_topk: logits [B][C]");
  const int B = logits.size(0), C = logits.size(1);
  check_dev(y, at::kLong, "y");
  check_dev(rank, at::kInt, "rank");
  TORCH_CHECK(y.numel() == B && loss.numel() == B && rank.numel() == B, "ce_topk: row counts");
  float* dl = optf32w(dlogits, "dlogits");
  if (dl) TORCH_CHECK(dlogits->numel() == (int64_t)B * C, "ce_topk: dlogits size");
  ce_topk(f32(logits, "logits"), y.data_ptr<int64_t>(), B, C, (float)gscale, f32w(loss, "loss"),
          rank.data_ptr<int>(), dl, cur_stream());
}

void class_sums_op(const Tensor& X, const Tensor& y, int64_t NC, const Tensor& sums,
                   const Tensor& counts) {
  TORCH_CHECK(X.dim() == 2, "class_sums: X [N][D]");
  const int N = X.size(0), D = X.size(1);
  check_dev(y, at::kLong, "y");
  TORCH_CHECK(y.numel() == N, "class_sums: labels");
  TORCH_CHECK(NC >= 1 && class_sums_lds((int)NC) <= 64 * 1024, "class_sums: at most ~250 classes");
  TORCH_CHECK(sums.numel() == NC * D && counts.numel() == NC, "class_sums: output sizes");
  const int G = class_sums_groups(N);
  at::Tensor part = at::empty({(int64_t)G * NC * D}, X.options());
  at::Tensor pcnt = at::empty({(int64_t)G * NC}, X.options());
  class_sums(f32(X, "X"), y.data_ptr<int64_t>(), N, D, (int)NC, part.data_ptr<float>(),
             pcnt.data_ptr<float>(), f32w(sums, "sums"), f32w(counts, "counts"), cur_stream());
}

// ------------------------------------------------------------------------------- k-NN probe
void knn_normalize_op(const Tensor& x, const Tensor& out) {
  TORCH_CHECK(x.dim() == 2 && out.dim() == 2, "knn_normalize: x [R][D], out [R][Dp]");
  TORCH_CHECK(x.scalar_type() == at::kFloat || x.scalar_type() == at::kBFloat16,
              "knn_normalize: x must be fp32 or bf16, got ", x.scalar_type());
  check_dev(x, x.scalar_type(), "x");
  const int64_t R = x.size(0), D = x.size(1), Dp = out.size(1);
  const int64_t ks = knn_kstep();
  TORCH_CHECK(R >= 1 && R < (1ll << 31) && D >= 1, "knn_normalize: empty input");
  TORCH_CHECK(out.size(0) == R && Dp == (D + ks - 1) / ks * ks && Dp <= 4096,
              "knn_normalize: out must be [R][D rounded up to ", ks, "] with Dp <= 4096, got [",
              out.size(0), "][", Dp, "] for D ", D);
  knn_normalize(x.data_ptr(), x.scalar_type() == at::kBFloat16, (int)R, (int)D, (int)Dp,
                bfw(out, "out"), cur_stream());
}

void knn_topk_op(const Tensor& qn, const Tensor& bn, int64_t k, bool exclude_self,
                 int64_t self_offset, const Tensor& vals, const Tensor& idx) {
  TORCH_CHECK(qn.dim() == 2 && bn.dim() == 2, "knn_topk: qn [Q][Dp], bn [N][Dp]");
  const int64_t Q = qn.size(0), N = bn.size(0), Dp = qn.size(1);
  TORCH_CHECK(bn.size(1) == Dp, "knn_topk: query and bank widths differ");
  TORCH_CHECK(Dp >= knn_kstep() && Dp % knn_kstep() == 0 && Dp <= 4096,
              "knn_topk: Dp must be a multiple of ", knn_kstep(), " and <= 4096, got ", Dp);
  TORCH_CHECK(Q >= 1 && N >= 1 && Q <= (1ll << 31) - 256 && N <= (1ll << 31) - 256,
              "knn_topk: Q and N must be in [1, 2^31 - 256]");
  TORCH_CHECK(k >= 1 && k <= knn_max_k(), "knn_topk: k must be in [1, ", knn_max_k(), "], got ", k);
  TORCH_CHECK(k <= N - (exclude_self ? 1 : 0), "knn_topk: k exceeds the selectable bank rows");
  TORCH_CHECK(self_offset > -(1ll << 40) && self_offset < (1ll << 40), "knn_topk: self_offset");
  TORCH_CHECK(knn_topk_lds() <= 160 * 1024, "knn_topk: LDS budget");
  TORCH_CHECK(vals.dim() == 2 && vals.size(0) == Q && vals.size(1) == k, "knn_topk: vals [Q][k]");
  TORCH_CHECK(idx.dim() == 2 && idx.size(0) == Q && idx.size(1) == k, "knn_topk: idx [Q][k]");
  check_dev(idx, at::kInt, "idx");
  const auto o = qn.options().dtype(at::kLong);
  at::Tensor buf = at::empty({(int64_t)knn_buf_keys((int)Q, (int)N)}, o);
  at::Tensor cand = at::empty({(int64_t)knn_cand_keys((int)Q, (int)N, (int)k)}, o);
  knn_topk(bf(qn, "qn"), bf(bn, "bn"), (int)Q, (int)N, (int)Dp, (int)k, exclude_self,
           (long long)self_offset, reinterpret_cast<unsigned long long*>(buf.data_ptr()),
           reinterpret_cast<unsigned long long*>(cand.data_ptr()), f32w(vals, "vals"),
           idx.data_ptr<int>(), cur_stream());
}

int64_t knn_scratch_bytes_op(int64_t Q, int64_t N, int64_t k) {
  TORCH_CHECK(Q >= 1 && N >= 1 && k >= 1 && Q < (1ll << 31) && N < (1ll << 31), "knn_scratch_bytes");
  return (int64_t)(8 * (knn_buf_keys((int)Q, (int)N) + knn_cand_keys((int)Q, (int)N, (int)k)));
}

void knn_vote_op(const Tensor& vals, const Tensor& idx, const Tensor& labels, int64_t C,
                 double temperature, const Tensor& targets, const Tensor& scores,
                 const Tensor& rank) {
  TORCH_CHECK(vals.dim() == 2 && idx.dim() == 2 && vals.sizes() == idx.sizes(),
              "knn_vote: vals and idx [Q][k]");
  const int64_t Q = vals.size(0), k = vals.size(1), N = labels.numel();
  TORCH_CHECK(Q >= 1 && Q < (1ll << 31) && N >= 1 && N < (1ll << 31), "knn_vote: Q, N");
  TORCH_CHECK(k >= 1 && k <= knn_max_k(), "knn_vote: k must be in [1, ", knn_max_k(), "]");
  TORCH_CHECK(C >= 1 && C <= knn_max_classes(), "knn_vote: num_classes must be in [1, ",
              knn_max_classes(), "], got ", C);
  TORCH_CHECK(temperature > 0.0, "knn_vote: temperature must be > 0");
  check_dev(idx, at::kInt, "idx");
  check_dev(labels, at::kLong, "labels");
  check_dev(targets, at::kLong, "targets");
  check_dev(rank, at::kInt, "rank");
  TORCH_CHECK(targets.numel() == Q && rank.numel() == Q, "knn_vote: targets / rank [Q]");
  TORCH_CHECK(scores.dim() == 2 && scores.size(0) == Q && scores.size(1) == C,
              "knn_vote: scores [Q][C]");
  knn_vote(f32(vals, "vals"), idx.data_ptr<int>(), labels.data_ptr<int64_t>(),
           targets.data_ptr<int64_t>(), (int)Q, (int)k, (int)N, (int)C, (float)(1.0 / temperature),
           f32w(scores, "scores"), rank.data_ptr<int>(), cur_stream());
}

// ------------------------------------------------------------------------------- k-means probe
// shared geometry checks: xn [N][Fp] bf16, cmat [R * Kp][Fp] bf16, a / s [R][N], counts [R * Kp],
// changed [R][Tp1], it [1]; every size is checked here, before any launch
struct KmGeom { int N, Fp, K, Kp, R, Tp1; };

KmGeom km_geometry(const char* op, const Tensor& xn, const Tensor& cmat, int64_t K, int64_t R,
                   const Tensor& a, const Tensor* s, const Tensor& counts, const Tensor* changed,
                   const Tensor* it, bool fit) {
  TORCH_CHECK(xn.dim() == 2 && cmat.dim() == 2, op, ": xn [N][Fp], cmat [R * Kp][Fp]");
  const int64_t N = xn.size(0), Fp = xn.size(1);
  TORCH_CHECK(Fp >= km_kstep() && Fp % km_kstep() == 0 && Fp <= km_max_fp(), op,
              ": Fp must be a multiple of ", km_kstep(), " and <= ", km_max_fp(), ", got ", Fp);
  TORCH_CHECK(N >= 1 && N * Fp < (1ll << 31), op, ": N must be >= 1 with N * Fp < 2^31, got N ", N,
              " Fp ", Fp);
  TORCH_CHECK(R >= 1 && R <= km_max_restarts(), op, ": R must be in [1, ", km_max_restarts(),
              "], got ", R);
  TORCH_CHECK(K >= 2 && K <= km_max_cols(), op, ": K must be in [2, ", km_max_cols(), "], got ", K);
  TORCH_CHECK(!fit || K <= N, op, ": K must be <= N, got K ", K, " N ", N);
  const int64_t Kp = (K + 15) / 16 * 16;
  TORCH_CHECK(R * Kp <= km_max_cols(), op, ": R * Kp must be <= ", km_max_cols(), ", got R ", R,
              " Kp ", Kp);
  TORCH_CHECK(cmat.size(0) == R * Kp && cmat.size(1) == Fp, op, ": cmat must be [R * Kp][Fp] = [",
              R * Kp, "][", Fp, "], got [", cmat.size(0), "][", cmat.size(1), "]");
  check_dev(a, at::kInt, "a");
  TORCH_CHECK(a.dim() == 2 && a.size(0) == R && a.size(1) == N, op, ": a must be [R][N]");
  if (s) TORCH_CHECK(s->dim() == 2 && s->size(0) == R && s->size(1) == N, op, ": s must be [R][N]");
  check_dev(counts, at::kInt, "counts");
  TORCH_CHECK(counts.numel() == R * Kp, op, ": counts must be [R * Kp]");
  int64_t Tp1 = 1;
  if (changed) {
    check_dev(*changed, at::kInt, "changed");
    TORCH_CHECK(changed->dim() == 2 && changed->size(0) == R && changed->size(1) >= 1, op,
                ": changed must be [R][iterations + 1]");
    Tp1 = changed->size(1);
  }
  if (it) {
    check_dev(*it, at::kInt, "it");
    TORCH_CHECK(it->numel() == 1, op, ": it must hold one int32");
  }
  return {(int)N, (int)Fp, (int)K, (int)Kp, (int)R, (int)Tp1};
}

void kmeans_assign_op(const Tensor& xn, const Tensor& cmat, int64_t K, int64_t R, const Tensor& a,
                      const Tensor& s, const Tensor& counts, const Tensor& changed,
                      const Tensor& it) {
  const KmGeom g = km_geometry("kmeans_assign", xn, cmat, K, R, a, &s, counts, &changed, &it, false);
  km_assign(bf(xn, "xn"), bf(cmat, "cmat"), g.N, g.Fp, g.K, g.Kp, g.R, a.data_ptr<int>(),
            f32w(s, "s"), counts.data_ptr<int>(), changed.data_ptr<int>(), it.data_ptr<int>(), g.Tp1,
            cur_stream());
}

void kmeans_update_op(const Tensor& xn, const Tensor& a, int64_t K, int64_t R, const Tensor& counts,
                      const Tensor& cmat, const c10::optional<Tensor>& S, const Tensor& it) {
  const KmGeom g = km_geometry("kmeans_update", xn, cmat, K, R, a, nullptr, counts, nullptr, &it,
                               false);
  float* Sp = optf32w(S, "S");
  TORCH_CHECK(!Sp || (S->dim() == 2 && S->size(0) == g.R * g.Kp && S->size(1) == g.Fp),
              "kmeans_update: S must be [R * Kp][Fp]");
  at::Tensor slab = at::empty({(int64_t)km_slab_floats(g.N, g.Fp, g.R * g.Kp)},
                              xn.options().dtype(at::kFloat));
  km_update(bf(xn, "xn"), a.data_ptr<int>(), g.N, g.Fp, g.K, g.Kp, g.R, counts.data_ptr<int>(),
            bfw(cmat, "cmat"), Sp, slab.data_ptr<float>(), it.data_ptr<int>(), cur_stream());
}

// T iterations of assign + update, the final assign and the objectives; nothing is read back and
// no launch argument depends on the iteration (the device counter `it` selects changed's column)
void kmeans_fit_op(const Tensor& xn, const Tensor& cmat, int64_t K, int64_t R, int64_t T,
                   const Tensor& a, const Tensor& s, const Tensor& counts, const Tensor& changed,
                   const Tensor& J) {
  TORCH_CHECK(T >= 1 && T <= 1000, "kmeans_fit: T must be in [1, 1000], got ", T);
  const KmGeom g = km_geometry("kmeans_fit", xn, cmat, K, R, a, &s, counts, &changed, nullptr, true);
  TORCH_CHECK(g.Tp1 == T + 1, "kmeans_fit: changed must be [R][T + 1]");
  check_dev(J, at::kDouble, "J");
  TORCH_CHECK(J.numel() == R, "kmeans_fit: J must be [R]");
  const uint16_t* X = bf(xn, "xn");
  uint16_t* C = bfw(cmat, "cmat");
  float* sp = f32w(s, "s");
  hipStream_t st = cur_stream();
  at::Tensor slab = at::empty({(int64_t)km_slab_floats(g.N, g.Fp, g.R * g.Kp)},
                              xn.options().dtype(at::kFloat));
  at::Tensor it = at::zeros({1}, xn.options().dtype(at::kInt));
  hipMemsetAsync(a.data_ptr(), 0xff, sizeof(int) * (size_t)g.R * g.N, st);  // -1: no assignment yet
  hipMemsetAsync(counts.data_ptr(), 0, sizeof(int) * (size_t)g.R * g.Kp, st);
  hipMemsetAsync(changed.data_ptr(), 0, sizeof(int) * (size_t)g.R * g.Tp1, st);
  for (int64_t t = 0; t <= T; ++t) {
    km_assign(X, C, g.N, g.Fp, g.K, g.Kp, g.R, a.data_ptr<int>(), sp, counts.data_ptr<int>(),
              changed.data_ptr<int>(), it.data_ptr<int>(), g.Tp1, st);
    if (t < T)
      km_update(X, a.data_ptr<int>(), g.N, g.Fp, g.K, g.Kp, g.R, counts.data_ptr<int>(), C, nullptr,
                slab.data_ptr<float>(), it.data_ptr<int>(), st);
  }
  km_objective(sp, g.R, g.N, J.data_ptr<double>(), st);
}

// ------------------------------------------------------------------------------- geometry probe
// rows N and padded width Dp of either half, checked before any launch
void geo_check_shape(const char* op, int64_t N, int64_t Dp) {
  TORCH_CHECK(N >= 2, op, ": N must be >= 2, got ", N);
  TORCH_CHECK(Dp >= geo_kstep() && Dp % geo_kstep() == 0 && Dp <= geo_max_dp(), op,
              ": Dp must be a multiple of ", geo_kstep(), " and <= ", geo_max_dp(), ", got ", Dp);
  TORCH_CHECK(N * Dp < (1ll << 31), op, ": N * Dp must be < 2^31, got N ", N, " Dp ", Dp);
}

void geometry_pair_op(const Tensor& xn, const c10::optional<Tensor>& labels, double t,
                      const Tensor& fpart, const Tensor& ipart) {
  TORCH_CHECK(xn.dim() == 2, "geometry_pair: xn [N][Dp]");
  const int64_t N = xn.size(0), Dp = xn.size(1);
  geo_check_shape("geometry_pair", N, Dp);
  TORCH_CHECK(N <= 128 * 65535, "geometry_pair: N must be <= ", 128 * 65535,
              " (the tile count of the triangle stays below 2^31), got ", N);
  TORCH_CHECK(t > 0.0 && std::isfinite(t), "geometry_pair: t must be > 0 and finite, got ", t);
  const int* lab = nullptr;
  if (labels.has_value() && labels->defined()) {
    check_dev(*labels, at::kInt, "labels");
    TORCH_CHECK(labels->numel() == N, "geometry_pair: labels must be [N]");
    lab = labels->data_ptr<int>();
  }
  const int64_t tiles = geo_pair_tiles((int)N);
  check_dev(ipart, at::kInt, "ipart");
  TORCH_CHECK(fpart.numel() == tiles * 3 && ipart.numel() == tiles * 2,
              "geometry_pair: fpart must be [", tiles, "][3] and ipart [", tiles, "][2]");
  geo_pair(bf(xn, "xn"), lab, (int)N, (int)Dp, (float)(2.0 * t), f32w(fpart, "fpart"),
           ipart.data_ptr<int>(), cur_stream());
}

void geometry_center_op(const Tensor& x, const Tensor& mu, const Tensor& cT) {
  TORCH_CHECK(x.dim() == 2 && cT.dim() == 2, "geometry_center: x [N][D], cT [Dp][Np]");
  const int64_t N = x.size(0), D = x.size(1), Dp = cT.size(0), Np = cT.size(1);
  const int64_t ks = geo_kstep();
  TORCH_CHECK(D >= 1 && Dp == (D + ks - 1) / ks * ks && Np == (N + 63) / 64 * 64,
              "geometry_center: cT must be [D rounded up to ", ks, "][N rounded up to 64], got [",
              Dp, "][", Np, "] for N ", N, " D ", D);
  geo_check_shape("geometry_center", N, Dp);
  TORCH_CHECK(mu.numel() == Dp, "geometry_center: mu must be [Dp]");
  const int64_t chunks = (N + geo_chunk() - 1) / geo_chunk();
  at::Tensor csum = at::empty({chunks * Dp}, x.options().dtype(at::kDouble));
  geo_center(f32(x, "x"), (int)N, (int)D, (int)Dp, (int)Np, csum.data_ptr<double>(),
             f32w(mu, "mu"), bfw(cT, "cT"), cur_stream());
}

void geometry_syrk_op(const Tensor& cT, int64_t N, const Tensor& S) {
  TORCH_CHECK(cT.dim() == 2, "geometry_syrk: cT [Dp][Np]");
  const int64_t Dp = cT.size(0), Np = cT.size(1);
  geo_check_shape("geometry_syrk", N, Dp);
  TORCH_CHECK(Np == (N + 63) / 64 * 64, "geometry_syrk: cT must be [Dp][N rounded up to 64]");
  check_dev(S, at::kDouble, "S");
  TORCH_CHECK(S.dim() == 2 && S.size(0) == Dp && S.size(1) == Dp, "geometry_syrk: S must be [Dp][Dp]");
  const int64_t slab_n = (int64_t)geo_syrk_splits((int)N, (int)Dp) * geo_syrk_tiles((int)Dp) * 4096;
  at::Tensor slab = at::empty({slab_n}, S.options());
  geo_syrk(bf(cT, "cT"), (int)N, (int)Dp, (int)Np, slab.data_ptr<double>(), S.data_ptr<double>(),
           cur_stream());
}

// ------------------------------------------------------------------------------- linear probes
// What the sweep and the online probe check alike: features [.][Fp] (bf16, contiguous: bf() checks
// where the pointer is taken) with Fp a multiple of the kernels' K step; returns Cp = 16 ceil(C / 16)
int64_t linear_probe_geometry(const char* op, const Tensor& X, int64_t C) {
  TORCH_CHECK(X.dim() == 2, op, ": features must be [rows][Fp]");
  const int64_t Fp = X.size(1);
  TORCH_CHECK(Fp >= probe_kstep() && Fp % probe_kstep() == 0 && Fp <= 4096, op,
              ": padded feature width must be a multiple of ", probe_kstep(), " and <= 4096, got ",
              Fp);
  TORCH_CHECK(C >= 1, op, ": C must be >= 1");
  return (C + 15) / 16 * 16;
}

// the forward's gradient outputs, NT columns in all: dlT [NT][ld >= Rp, a multiple of 32] (returns
// ld), dbp [>= RT][NT] (one row per 16-row tile)
int64_t linear_probe_grad_bufs(const char* op, const Tensor& dlT, const Tensor& dbp, int64_t NT,
                               int64_t Rp, int64_t RT) {
  TORCH_CHECK(dlT.dim() == 2 && dlT.size(0) == NT && dlT.size(1) >= Rp && dlT.size(1) % 32 == 0, op,
              ": dlT [", NT, "][>= rows rounded up to 32, a multiple of 32]");
  TORCH_CHECK(dbp.numel() >= RT * NT, op, ": dbp [", RT, "][", NT, "]");
  return dlT.size(1);
}

// ------------------------------------------------------------------------------- probe sweep
// the sweep's own: X [N][Fp], idx [rows] int64, G configurations of C classes
int64_t probe_geometry(const char* op, const Tensor& X, const Tensor& idx, const Tensor& Wsh,
                       int64_t G, int64_t C) {
  const int64_t Cp = linear_probe_geometry(op, X, C);
  const int64_t N = X.size(0), Fp = X.size(1), rows = idx.numel();
  TORCH_CHECK(N >= 1 && N < (1ll << 31), op, ": N must be in [1, 2^31)");
  TORCH_CHECK(G >= 1 && G <= probe_max_configs(), op, ": G must be in [1, ", probe_max_configs(),
              "], got ", G);
  TORCH_CHECK(G * Cp <= probe_max_cols(), op, ": G * Cp must be <= ", probe_max_cols(), ", got ",
              G * Cp);
  TORCH_CHECK(rows >= 1 && rows <= probe_max_rows(), op, ": rows must be in [1, ",
              probe_max_rows(), "], got ", rows);
  TORCH_CHECK(Wsh.dim() == 2 && Wsh.size(0) == G * Cp && Wsh.size(1) == Fp, op, ": Wsh must be [",
              G * Cp, "][", Fp, "]");
  check_dev(idx, at::kLong, "idx");
  return Cp;
}

void probe_forward_op(const Tensor& X, const Tensor& y, const Tensor& idx, const Tensor& Wsh,
                      const Tensor& bias, int64_t G, int64_t C, const Tensor& Z,
                      const Tensor& loss, int64_t loss_stride, const c10::optional<Tensor>& rank,
                      const c10::optional<Tensor>& dlT, const c10::optional<Tensor>& dbp) {
  const int64_t Cp = probe_geometry("probe_forward", X, idx, Wsh, G, C);
  const int64_t N = X.size(0), rows = idx.numel(), NT = G * Cp;
  const bool train = dlT.has_value() && dlT->defined();
  const int64_t Rp = train ? (rows + 31) / 32 * 32 : (rows + 15) / 16 * 16;
  check_dev(y, at::kLong, "y");
  TORCH_CHECK(y.numel() == N, "probe_forward: y [N]");
  TORCH_CHECK(bias.numel() == NT, "probe_forward: bias [G * Cp]");
  TORCH_CHECK(Z.numel() >= rows * NT, "probe_forward: logits scratch [rows][G * Cp]");
  TORCH_CHECK(loss_stride >= rows && loss.numel() >= (G - 1) * loss_stride + rows,
              "probe_forward: loss [G][loss_stride >= rows]");
  ProbeFwdArgs a{};
  a.X = bf(X, "X");
  a.y = y.data_ptr<int64_t>();
  a.idx = idx.data_ptr<int64_t>();
  a.N = N;
  a.Fp = (int)X.size(1);
  a.rows = (int)rows;
  a.Rp = (int)Rp;
  a.G = (int)G;
  a.C = (int)C;
  a.Cp = (int)Cp;
  a.Wsh = bf(Wsh, "Wsh");
  a.bias = f32(bias, "bias");
  a.Z = f32w(Z, "Z");
  a.loss = f32w(loss, "loss");
  a.loss_stride = loss_stride;
  if (rank.has_value() && rank->defined()) {
    check_dev(*rank, at::kInt, "rank");
    TORCH_CHECK(rank->numel() == G * rows, "probe_forward: rank [G][rows]");
    a.rank = rank->data_ptr<int>();
  }
  if (train) {
    TORCH_CHECK(dbp.has_value() && dbp->defined(), "probe_forward: dbp goes with dlT");
    a.ldr = (int)linear_probe_grad_bufs("probe_forward", *dlT, *dbp, NT, Rp, (rows + 15) / 16);
    a.dlT = bfw(*dlT, "dlT");
    a.dbp = f32w(*dbp, "dbp");
  }
  probe_forward(a, cur_stream());
}

void probe_update_op(const Tensor& X, const Tensor& idx, const Tensor& dlT, const Tensor& dbp,
                     const Tensor& W, const Tensor& Mw, const Tensor& Wsh, const Tensor& b,
                     const Tensor& Mb, const Tensor& lr0, const Tensor& wd, const Tensor& ftab,
                     int64_t step, double momentum, int64_t G, int64_t C) {
  const int64_t Cp = probe_geometry("probe_update", X, idx, Wsh, G, C);
  const int64_t rows = idx.numel(), NT = G * Cp, Fp = X.size(1);
  const int64_t Rp = (rows + 31) / 32 * 32;
  const int64_t ldr = linear_probe_grad_bufs("probe_update", dlT, dbp, NT, Rp, (rows + 15) / 16);
  TORCH_CHECK(W.numel() == NT * Fp && Mw.numel() == NT * Fp, "probe_update: W, Mw [G * Cp][Fp]");
  TORCH_CHECK(b.numel() == NT && Mb.numel() == NT, "probe_update: b, Mb [G * Cp]");
  TORCH_CHECK(lr0.numel() == G && wd.numel() == G, "probe_update: lr0, wd [G]");
  TORCH_CHECK(step >= 0 && step < ftab.numel(), "probe_update: step ", step,
              " outside the schedule table of ", ftab.numel());
  ProbeUpdArgs a{};
  a.X = bf(X, "X");
  a.idx = idx.data_ptr<int64_t>();
  a.N = X.size(0);
  a.Fp = (int)Fp;
  a.rows = (int)rows;
  a.Rp = (int)Rp;
  a.G = (int)G;
  a.C = (int)C;
  a.Cp = (int)Cp;
  a.dlT = bf(dlT, "dlT");
  a.ldr = (int)ldr;
  a.dbp = f32(dbp, "dbp");
  a.W = f32w(W, "W");
  a.Mw = f32w(Mw, "Mw");
  a.b = f32w(b, "b");
  a.Mb = f32w(Mb, "Mb");
  a.Wsh = bfw(Wsh, "Wsh");
  a.lr0 = f32(lr0, "lr0");
  a.wd = f32(wd, "wd");
  a.ftab = f32(ftab, "ftab");
  a.step = (int)step;
  a.momentum = (float)momentum;
  probe_update(a, cur_stream());
}

// ------------------------------------------------------------------------------- online probe
// the online probe's own: h [rows][Fp] with rows = 2n a multiple of 16, one configuration, and
// dlT exactly [Cp][Rp]
struct OnlineProbeGeom {
  int64_t rows, Rp, Fp, Cp;
};
OnlineProbeGeom online_probe_geometry(const char* op, const Tensor& h, int64_t C) {
  const int64_t Cp = linear_probe_geometry(op, h, C);
  OnlineProbeGeom g{h.size(0), (h.size(0) + 31) / 32 * 32, h.size(1), Cp};
  TORCH_CHECK(g.rows >= 16 && g.rows % 16 == 0 && g.rows <= online_probe_max_rows(), op,
              ": rows must be a multiple of 16 in [16, ", online_probe_max_rows(), "], got ",
              g.rows);
  TORCH_CHECK(g.Cp <= online_probe_max_cols(), op, ": C must be in [1, ", online_probe_max_cols(),
              "], got ", C);
  return g;
}
void online_probe_grad_bufs(const char* op, const OnlineProbeGeom& g, const Tensor& dlT,
                            const Tensor& dbp) {
  const int64_t ld = linear_probe_grad_bufs(op, dlT, dbp, g.Cp, g.Rp, g.rows / 16);
  TORCH_CHECK(ld == g.Rp, op, ": dlT [Cp][rows rounded up to 32]");
}

void online_probe_forward_op(const Tensor& h, const Tensor& y, const Tensor& Wsh,
                             const Tensor& bias, int64_t C, const Tensor& Z, const Tensor& loss,
                             const Tensor& rank, const Tensor& dlT, const Tensor& dbp) {
  const char* op = "online_probe_forward";
  const OnlineProbeGeom g = online_probe_geometry(op, h, C);
  const int64_t n = y.numel();
  TORCH_CHECK(n >= 1 && g.rows % n == 0, op, ": y [n] with rows a multiple of n, got rows ",
              g.rows, " and n ", n);
  TORCH_CHECK(Wsh.dim() == 2 && Wsh.size(0) == g.Cp && Wsh.size(1) == g.Fp, op, ": Wsh must be [",
              g.Cp, "][", g.Fp, "]");
  TORCH_CHECK(bias.numel() == g.Cp, op, ": bias [Cp]");
  TORCH_CHECK(Z.numel() >= g.rows * g.Cp, op, ": logits scratch [rows][Cp]");
  TORCH_CHECK(loss.numel() == g.rows && rank.numel() == g.rows, op, ": loss, rank [rows]");
  online_probe_grad_bufs(op, g, dlT, dbp);
  check_dev(rank, at::kInt, "rank");
  OnlineProbeFwdArgs a{};
  a.X = bf(h, "h");
  a.y = i32(y, "y");
  a.n = (int)n;
  a.rows = (int)g.rows;
  a.Rp = (int)g.Rp;
  a.Fp = (int)g.Fp;
  a.C = (int)C;
  a.Cp = (int)g.Cp;
  a.Wsh = bf(Wsh, "Wsh");
  a.bias = f32(bias, "bias");
  a.Z = f32w(Z, "Z");
  a.loss = f32w(loss, "loss");
  a.rank = rank.data_ptr<int>();
  a.dlT = bfw(dlT, "dlT");
  a.dbp = f32w(dbp, "dbp");
  online_probe_forward(a, cur_stream());
}

void online_probe_metrics_op(const Tensor& loss, const Tensor& rank, int64_t top_k,
                             const Tensor& acc_loss, const Tensor& acc_cnt) {
  const char* op = "online_probe_metrics";
  check_dev(rank, at::kInt, "rank");
  check_dev(acc_loss, at::kDouble, "acc_loss");
  check_dev(acc_cnt, at::kLong, "acc_cnt");
  TORCH_CHECK(loss.numel() == rank.numel() && loss.numel() >= 1 &&
                  loss.numel() <= online_probe_max_rows(),
              op, ": loss, rank [rows], rows in [1, ", online_probe_max_rows(), "]");
  TORCH_CHECK(top_k >= 1, op, ": top_k must be >= 1, got ", top_k);
  TORCH_CHECK(acc_loss.numel() == 1 && acc_cnt.numel() == 3, op, ": acc_loss [1], acc_cnt [3]");
  online_probe_metrics(f32(loss, "loss"), rank.data_ptr<int>(), (int)loss.numel(),
                       (int)std::min<int64_t>(top_k, 1 << 30), acc_loss.data_ptr<double>(),
                       reinterpret_cast<long long*>(acc_cnt.data_ptr<int64_t>()), cur_stream());
}

void online_probe_wgrad_op(const Tensor& h, const Tensor& dlT, const Tensor& dbp,
                           const Tensor& grad, int64_t C) {
  const char* op = "online_probe_wgrad";
  const OnlineProbeGeom g = online_probe_geometry(op, h, C);
  online_probe_grad_bufs(op, g, dlT, dbp);
  TORCH_CHECK(grad.numel() == g.Cp * g.Fp + g.Cp, op, ": grad [Cp * Fp + Cp]");
  OnlineProbeGradArgs a{};
  a.X = bf(h, "h");
  a.rows = (int)g.rows;
  a.Rp = (int)g.Rp;
  a.Fp = (int)g.Fp;
  a.Cp = (int)g.Cp;
  a.dlT = bf(dlT, "dlT");
  a.dbp = f32(dbp, "dbp");
  a.grad = f32w(grad, "grad");
  online_probe_wgrad(a, cur_stream());
}

void online_probe_update_op(const Tensor& master, const Tensor& grad, const Tensor& mom,
                            const Tensor& shadow, const Tensor& lr, double wd, double momentum,
                            double gscale, int64_t C, int64_t F, int64_t Fp) {
  const char* op = "online_probe_update";
  const int64_t Cp = (C + 15) / 16 * 16;
  TORCH_CHECK(C >= 1 && Cp <= online_probe_max_cols(), op, ": C must be in [1, ",
              online_probe_max_cols(), "], got ", C);
  TORCH_CHECK(Fp >= online_probe_kstep() && Fp % online_probe_kstep() == 0 &&
                  Fp <= online_probe_max_fp() && F >= 1 && F <= Fp,
              op, ": F in [1, Fp], Fp a multiple of ", online_probe_kstep(), " and <= ",
              online_probe_max_fp(), ", got F ", F, " Fp ", Fp);
  const int64_t total = Cp * Fp + Cp;
  TORCH_CHECK(master.numel() == total && grad.numel() == total && mom.numel() == total, op,
              ": master, grad, mom [Cp * Fp + Cp]");
  TORCH_CHECK(shadow.numel() == Cp * Fp, op, ": shadow [Cp][Fp]");
  TORCH_CHECK(lr.numel() == 1, op, ": lr [1]");
  OnlineProbeUpdArgs a{};
  a.master = f32w(master, "master");
  a.mom = f32w(mom, "mom");
  a.grad = f32(grad, "grad");
  a.shadow = bfw(shadow, "shadow");
  a.lr = f32(lr, "lr");
  a.wd = (float)wd;
  a.momentum = (float)momentum;
  a.gscale = (float)gscale;
  a.C = (int)C;
  a.Cp = (int)Cp;
  a.F = (int)F;
  a.Fp = (int)Fp;
  online_probe_update(a, cur_stream());
}

}  // namespace


TORCH_LIBRARY(simclr_amd, m) {
  m.def("probe_forward(Tensor X, Tensor y, Tensor idx, Tensor Wsh, Tensor bias, int G, int C, Tensor(a!) Z, Tensor(b!) loss, int loss_stride, Tensor(c!)? rank, Tensor(d!)? dlT, Tensor(e!)? dbp) -> ()", &probe_forward_op);
  m.def("probe_update(Tensor X, Tensor idx, Tensor dlT, Tensor dbp, Tensor(a!) W, Tensor(b!) Mw, Tensor(c!) Wsh, Tensor(d!) b, Tensor(e!) Mb, Tensor lr0, Tensor wd, Tensor ftab, int step, float momentum, int G, int C) -> ()", &probe_update_op);
  m.def("online_probe_forward(Tensor h, Tensor y, Tensor Wsh, Tensor bias, int C, Tensor(a!) Z, Tensor(b!) loss, Tensor(c!) rank, Tensor(d!) dlT, Tensor(e!) dbp) -> ()", &online_probe_forward_op);
  m.def("online_probe_metrics(Tensor loss, Tensor rank, int top_k, Tensor(a!) acc_loss, Tensor(b!) acc_cnt) -> ()", &online_probe_metrics_op);
  m.def("online_probe_wgrad(Tensor h, Tensor dlT, Tensor dbp, Tensor(a!) grad, int C) -> ()", &online_probe_wgrad_op);
  m.def("online_probe_update(Tensor(a!) master, Tensor grad, Tensor(b!) mom, Tensor(c!) shadow, Tensor lr, float wd, float momentum, float gscale, int C, int F, int Fp) -> ()", &online_probe_update_op);
  m.def("knn_normalize(Tensor x, Tensor(a!) out) -> ()", &knn_normalize_op);
  m.def("knn_topk(Tensor qn, Tensor bn, int k, bool exclude_self, int self_offset, Tensor(a!) vals, Tensor(b!) idx) -> ()", &knn_topk_op);
  m.def("knn_scratch_bytes(int Q, int N, int k) -> int", &knn_scratch_bytes_op);
  m.def("knn_kstep() -> int", []() -> int64_t { return knn_kstep(); });
  m.def("knn_vote(Tensor vals, Tensor idx, Tensor labels, int C, float temperature, Tensor targets, Tensor(a!) scores, Tensor(b!) rank) -> ()", &knn_vote_op);
  m.def("kmeans_assign(Tensor xn, Tensor cmat, int K, int R, Tensor(a!) a, Tensor(b!) s, Tensor(c!) counts, Tensor(d!) changed, Tensor it) -> ()", &kmeans_assign_op);
  m.def("kmeans_update(Tensor xn, Tensor a, int K, int R, Tensor(a!) counts, Tensor(b!) cmat, Tensor(c!)? S, Tensor(d!) it) -> ()", &kmeans_update_op);
  m.def("kmeans_fit(Tensor xn, Tensor(a!) cmat, int K, int R, int T, Tensor(b!) a, Tensor(c!) s, Tensor(d!) counts, Tensor(e!) changed, Tensor(f!) J) -> ()", &kmeans_fit_op);
  m.def("geometry_pair(Tensor xn, Tensor? labels, float t, Tensor(a!) fpart, Tensor(b!) ipart) -> ()", &geometry_pair_op);
  m.def("geometry_pair_tiles(int N) -> int", [](int64_t N) -> int64_t { return geo_pair_tiles((int)N); });
  m.def("geometry_pair_chain() -> int", []() -> int64_t { return geo_pair_chain(); });
  m.def("geometry_center(Tensor x, Tensor(a!) mu, Tensor(b!) cT) -> ()", &geometry_center_op);
  m.def("geometry_syrk(Tensor cT, int N, Tensor(a!) S) -> ()", &geometry_syrk_op);
  m.def("geometry_syrk_splits(int N, int Dp) -> int", [](int64_t N, int64_t Dp) -> int64_t { return geo_syrk_splits((int)N, (int)Dp); });
  m.def("maxpool_fwd(Tensor x, Tensor(a!) y, Tensor(b!) arg, int K, int S, int P) -> ()", &maxpool_fwd_op);
  m.def("maxpool_bwd(Tensor dy, Tensor arg, Tensor(a!) dx, int K, int S, int P) -> ()", &maxpool_bwd_op);
  m.def("stem_s2d(Tensor img, int creal, int P, Tensor(a!) xs) -> ()", &stem_s2d_op);
  m.def("gemm_sk(Tensor A, Tensor B, Tensor? sc, Tensor? sh, int seg, int KS, Tensor(a!) part, "
        "Tensor? bias, Tensor(b!) out) -> ()", &gemm_sk_op);
  m.def("bn_relu_maxpool(Tensor a, Tensor ss, int S, Tensor(a!) y, Tensor(b!) arg, Tensor(c!) asel, "
        "int K, int Sd, int P) -> ()", &bn_relu_maxpool_op);
  m.def("maxpool_bwd_bn(Tensor gy, Tensor arg, Tensor y, Tensor a, Tensor coef, int S, Tensor(a!) da, "
        "int K, int Sd, int P) -> ()", &maxpool_bwd_bn_op);
  m.def("ce_topk(Tensor logits, Tensor y, float gscale, Tensor(a!) loss, Tensor(b!) rank, Tensor(c!)? dlogits=None) -> ()", &ce_topk_op);
  m.def("class_sums(Tensor X, Tensor y, int NC, Tensor(a!) sums, Tensor(b!) counts) -> ()", &class_sums_op);
  m.def("igemm(Tensor A, Tensor B, Tensor(a!) out, Tensor? bias, Tensor(b!)? stats, int[] geom, Tensor? pro_sc=None, Tensor? pro_sh=None, int pro_seg_rows=0, bool pro_relu=False, int epi_mode=0, Tensor? epi_a=None, Tensor? epi_b=None, int variant=-1, Tensor? epi_ss=None, Tensor? epi_mi=None, int seg_rows=0, int stats_seg_blocks=0, int stats_base=0, Tensor? epi_c=None, Tensor? epi_mask=None, Tensor? epi_c2=None, Tensor? epi_mi2=None, Tensor(c!)? stats2=None, Tensor? pro_d=None, Tensor? A2=None, Tensor? pro_rss=None, Tensor(d!)? pro_out=None, Tensor(e!)? pro_mask=None) -> ()", &igemm);
  m.def("igemm_dual_ok(int v, int[] geom) -> bool", &igemm_dok);
  m.def("igemm_bm(int N) -> int", &igemm_bm);
  m.def("igemm_nvariants() -> int", &igemm_nvariants);
  m.def("igemm_variant_bm(int v) -> int", &igemm_vbm);
  m.def("igemm_variant_bn(int v) -> int", &igemm_vbn);
  m.def("igemm_variant_glds(int v) -> bool", &igemm_vglds);
  m.def("igemm_glds_ok(int[] geom, bool pro, bool bn_bwd_pro) -> bool", &igemm_gldsok);
  m.def("wgrad_nvariants() -> int", &wgrad_nvariants);
  m.def("wgrad_xlin(int mode=-1) -> int", &wgrad_xlin_op);
  m.def("wgrad_variant_glds(int v) -> bool", &wgrad_vglds);
  m.def("igemm_variant_patch(int v) -> bool", [](int64_t v) { return igemm_variant_patch((int)v); });
  m.def("wgrad_variant_area(int v) -> int", [](int64_t v) -> int64_t {
    TORCH_CHECK(v >= 0 && v < wgrad_num_variants(), "wgrad variant out of range");
    return wgrad_variant_area((int)v);
  });
  m.def("igemm_variant_ok(int v, int[] geom, bool pro, bool bn_bwd_pro, int epi_mode=0) -> bool",
        &igemm_vok);
  m.def("wgrad_variant_ok(int v, int[] geom, bool pro, bool dy_pro) -> bool", &wgrad_vok);
  m.def("wgrad_splits(int[] geom, int variant=-1) -> int", &wgrad_nsplit);
  m.def("wgrad_tiles(int[] geom, int variant=-1) -> int", &wgrad_ntiles);
  m.def("conv1x1_bwd_dual_s2(Tensor G, Tensor? A3, Tensor? coef, Tensor X, Tensor Wt, "
        "Tensor(a!) gm, Tensor(b!) wpart, int S, int bps) -> ()", &conv1x1_bwd_dual_s2_op);
  m.def("conv1x1_bwd_dual(Tensor G, Tensor? A3, Tensor? coef, Tensor X, Tensor? xss, Tensor? xmi, Tensor Wt, Tensor(a!) gm, Tensor(b!) stats, Tensor(c!) wpart, int S, int bps, Tensor? Xraw=None, bool dual8=False) -> ()", &conv1x1_bwd_dual_op);
  m.def("wgrad_reduce_slabs(Tensor(a!) partial, int splits, Tensor(b!) out, float beta=0.0) -> ()", &wgrad_reduce_slabs_op);
  m.def("wgrad(Tensor dY, Tensor X, Tensor(a!) partial, Tensor(b!) out, int[] geom, int splits, int creal, float beta, Tensor? pro_sc=None, Tensor? pro_sh=None, int pro_seg_rows=0, bool pro_relu=False, int pro_S=1, int variant=-1, Tensor? dY2=None, Tensor? dp_coef=None, int dp_seg_rows=0, int dp_S=1) -> ()", &wgrad);
  m.def("weight_transform(Tensor W, Tensor(a!) Wt, int[] p) -> ()", &weight_transform);
  m.def("weight_transform_plan(Tensor[] Ws, Tensor[] Wts, int[] p) -> Tensor", &weight_transform_plan);
  m.def("weight_transform_batch(Tensor table, int total_blocks) -> ()", &weight_transform_batch);
  m.def("bn_blocks(int R, int C, int S) -> int", &bn_blocks);
  m.def("bn_stats(Tensor x, int S, Tensor(a!) partial) -> ()", &bn_stats);
  m.def("bn_reduce(Tensor partial, int nblk, int S, int C, Tensor(a!) stats) -> ()", &bn_reduce);
  m.def("bn_finalize(Tensor stats, int S, int C, float count, float eps, float momentum, Tensor(a!)? rm, Tensor(b!)? rv, Tensor(c!) mi, Tensor(d!)? nbt, Tensor? gamma=None, Tensor? beta=None, Tensor(e!)? ss=None) -> ()", &bn_final);
  m.def("ipc_collective(int op, Tensor src, Tensor(a!) dst, Tensor peers, Tensor(b!) arena, int site, Tensor(c!) epoch, Tensor(d!) err, int world, int rank) -> ()", &ipc_collective_op);
  m.def("ipc_coll_blocks() -> int", []() -> int64_t { return IPC_COLL_BLOCKS; });
  m.def("bn_reduce_fused(Tensor partial, int nblk, int S, int C, int mode, Tensor(a!)? stats=None, float count=1.0, float eps=1e-5, float momentum=0.1, Tensor(b!)? rm=None, Tensor(c!)? rv=None, Tensor(d!)? mi=None, Tensor(e!)? nbt=None, Tensor? gamma=None, Tensor? beta=None, Tensor(f!)? ss=None, Tensor(g!)? dgamma=None, Tensor(h!)? dbeta=None, Tensor(i!)? coef=None, int ticket_slot=0, Tensor? ipc_peers=None, Tensor(j!)? ipc_arena=None, int ipc_site=0, Tensor(k!)? ipc_epoch=None, Tensor(l!)? ipc_err=None, int world=1, int rank=0) -> ()", &bn_reduce_fused_op);
  // the ticket arrays are allocated outside any capture: Trainer.capture() calls this first
  m.def("bn_tickets_init(Tensor like) -> ()", [](const Tensor& like) { (void)tickets_for(like, 0, 0); });
  m.def("bn_apply_ss(Tensor x, Tensor ss, Tensor? res, Tensor? rss, Tensor(a!) y, int S, bool relu, Tensor(b!)? mask=None) -> ()", &bn_apply_ss_op);
  m.def("bn_apply(Tensor x, Tensor? res, Tensor(a!) y, Tensor mi, Tensor? gamma, Tensor? beta, int S, bool relu) -> ()", &bn_apply_op);
  m.def("bn_apply_eval(Tensor x, Tensor? res, Tensor(a!) y, Tensor rm, Tensor rv, Tensor? gamma, Tensor? beta, float eps, bool relu) -> ()", &bn_apply_eval_op);
  m.def("bn_bwd_reduce(Tensor dy, Tensor? y, Tensor x, Tensor mi, int S, bool relu, Tensor(a!) partial) -> ()", &bn_bwd_reduce_op);
  m.def("bn_bwd_finalize(Tensor sums, Tensor mi, Tensor? gamma, int S, int C, float count, Tensor(a!)? dgamma, Tensor(b!)? dbeta, Tensor(c!) coef) -> ()", &bn_bwd_final);
  m.def("bn_bwd_apply(Tensor dy, Tensor? y, Tensor x, Tensor coef, int S, bool relu, Tensor(a!) dx, Tensor(b!)? dres) -> ()", &bn_bwd_apply_op);
  m.def("bn_bwd_apply2(Tensor g, Tensor x1, Tensor coef1, Tensor(a!) dx1, Tensor x2, Tensor coef2, Tensor(b!) dx2, int S) -> ()", &bn_bwd_apply2_op);
  m.def("avgpool_fwd(Tensor x, Tensor(a!) y, int Nb, int HW, int C) -> ()", &avgpool_fwd_op);
  m.def("avgpool_bwd(Tensor dy, Tensor(a!) dx, int Nb, int HW, int C) -> ()", &avgpool_bwd_op);
  m.def("colsum(Tensor x, Tensor(a!) out, float beta) -> ()", &colsum_op);
  m.def("cast_to_bf16(Tensor x, Tensor(a!) y) -> ()", &cast_to_bf16);
  m.def("cast_to_f32(Tensor x, Tensor(a!) y) -> ()", &cast_to_f32);
  m.def("nt_normalize(Tensor z, Tensor(a!) zn, Tensor(b!) inv_norm) -> ()", &nt_normalize);
  m.def("nt_transpose(Tensor x, Tensor(a!) out) -> ()", &nt_transpose);
  m.def("nt_transpose_cols(Tensor x, Tensor(a!) out, int c0) -> ()", &nt_transpose_cols);
  m.def("nt_forward_range(Tensor znT, int R, int col_offset, int n_local, float inv_temp, Tensor(a!) part, int c_lo, int c_hi, int splits, int split_base) -> ()", &nt_forward_range);
  m.def("nt_finish(Tensor part, int R, int splits, Tensor(a!) lse, Tensor(b!) loss) -> ()", &nt_finish);
  m.def("nt_fwd_splits(int R, int C) -> int", &nt_fwd_splits);
  m.def("nt_bwd_splits(int nown, int npart) -> int", &nt_bwd_splits);
  m.def("nt_forward(Tensor znT, int R, int col_offset, int n_local, float inv_temp, Tensor(a!) part, int splits, Tensor(b!) lse, Tensor(c!) loss) -> ()", &nt_forward);
  m.def("nt_backward_part(bool row_mode, Tensor zn, Tensor znT, Tensor lse, int R, int col_offset, int n_local, float inv_temp, float gscale, Tensor? gout, Tensor(a!) part, int splits, Tensor(b!) out) -> ()", &nt_backward_part);
  m.def("nt_normalize_backward(Tensor zn, Tensor inv_norm, Tensor dzn, Tensor(a!)? dz_bf16, Tensor(b!)? dz_f32) -> ()", &nt_normalize_backward);
  m.def("nt_reduce_loss(Tensor loss_rows, float scale, Tensor(a!) out) -> ()", &nt_reduce_loss);
  m.def("nt_w_forward_range(Tensor znT, int R, int col_offset, int n_local, float inv_temp, float hard_beta, Tensor(a!) part, int c_lo, int c_hi, int splits, int split_base) -> ()", &nt_w_forward_range);
  m.def("nt_w_finish(Tensor part, int R, int splits, int Ccols, float inv_temp, float hard_beta, float tau_plus, bool decoupled, Tensor(a!) stats, Tensor(b!) loss) -> ()", &nt_w_finish);
  m.def("nt_w_backward_part(bool row_mode, Tensor zn, Tensor znT, Tensor stats, int R, int col_offset, int n_local, float inv_temp, float hard_beta, float gscale, Tensor? gout, Tensor(a!) part, int splits, Tensor(b!) out) -> ()", &nt_w_backward_part);
  m.def("nt_sup_forward_range(Tensor znT, Tensor ycol, int y0, int R, int col_offset, int n_local, float inv_temp, Tensor(a!) part, int c_lo, int c_hi, int splits, int split_base) -> ()", &nt_sup_forward_range);
  m.def("nt_sup_finish(Tensor part, int R, int splits, Tensor(a!) lse, Tensor(b!) inv_cnt, Tensor(c!) loss) -> ()", &nt_sup_finish);
  m.def("nt_sup_backward_part(bool row_mode, Tensor zn, Tensor znT, Tensor lse, Tensor inv_cnt, Tensor ycol, int R, int col_offset, int n_local, float inv_temp, float gscale, Tensor? gout, Tensor(a!) part, int splits, Tensor(b!) out) -> ()", &nt_sup_backward_part);
  m.def("nt_expand_labels(Tensor labels, Tensor? idx, int views, Tensor(a!) out) -> ()", &nt_expand_labels);
  m.def("nc_top1_splits(int R, int Q) -> int", &nc_top1_splits);
  m.def("nc_loss_splits(int n) -> int", &nc_loss_splits);
  m.def("nc_normalize(Tensor z, Tensor(a!) zn, Tensor(b!) zb, Tensor(c!) inv_norm) -> ()", &nc_normalize);
  m.def("nc_lookup(Tensor zb, Tensor queue, int splits, Tensor(a!) candv, Tensor(b!) candi, Tensor(c!) idx, Tensor(d!) a) -> ()", &nc_lookup);
  m.def("nc_forward(Tensor a, Tensor zb, float inv_temp, int splits, Tensor(a!) part) -> ()", &nc_forward);
  m.def("nc_backward(Tensor a, Tensor zb, Tensor zn, Tensor inv_norm, Tensor lse, float inv_temp, Tensor gout, int splits, Tensor(a!) part, Tensor(b!)? dz_bf16, Tensor(c!)? dz_f32) -> ()", &nc_backward);
  m.def("nc_enqueue(Tensor zb, Tensor(a!) queue, Tensor(b!) cursor) -> ()", &nc_enqueue);
  m.def("bt_standardize(Tensor z, float eps, Tensor(a!) rstd, Tensor(b!) zh, Tensor(c!) zhT) -> ()", &bt_standardize);
  m.def("bt_corr_splits(int n, int D) -> int", &bt_corr_splits);
  m.def("bt_loss_blocks(int D) -> int", &bt_loss_blocks);
  m.def("bt_corr(Tensor zhT, int n, int splits, Tensor(a!) part) -> ()", &bt_corr);
  m.def("bt_loss(Tensor part, int splits, int n, float lambd, Tensor(a!) C, Tensor(b!) lpart) -> ()", &bt_loss);
  m.def("bt_grad(Tensor C, float lambd, Tensor gout, Tensor(a!) G, Tensor(b!) GT) -> ()", &bt_grad);
  m.def("bt_backward(Tensor zh, Tensor G, Tensor GT, Tensor(a!) dzh, Tensor(b!) colpart) -> ()", &bt_backward);
  m.def("bt_std_backward(Tensor zh, Tensor rstd, Tensor dzh, Tensor colpart, Tensor(a!)? dz_bf16, Tensor(b!)? dz_f32) -> ()", &bt_std_backward);
  m.def("bt_stats(Tensor z, Tensor(a!) stats) -> ()", &bt_stats);
  m.def("bt_merge_standardize(Tensor z, Tensor gstats, float eps, Tensor(a!) rstd, Tensor(b!) zh, Tensor(c!) zhT) -> ()", &bt_merge_standardize);
  m.def("bt_slab_merge(Tensor part, int splits, Tensor(a!) S) -> ()", &bt_slab_merge);
  m.def("bt_colsum(Tensor colpart, Tensor(a!) csum) -> ()", &bt_colsum);
  m.def("bt_std_backward_global(Tensor zh, Tensor rstd, Tensor dzh, Tensor gsum, Tensor(a!)? dz_bf16, Tensor(b!)? dz_f32) -> ()", &bt_std_backward_global);
  m.def("lars_norms(Tensor p, Tensor g, Tensor chunk_beg, Tensor chunk_end, float grad_scale, Tensor(a!) norms) -> ()", &lars_norms_op);
  m.def("lars_update(Tensor(a!) p, Tensor g, Tensor(b!) mom, Tensor(c!)? shadow, Tensor chunk_seg, Tensor chunk_beg, Tensor chunk_end, Tensor seg_chunk_beg, Tensor seg_chunk_end, Tensor seg_wd, Tensor seg_flags, Tensor norms, Tensor lr, float momentum, float trust, float eps, float grad_scale, bool nesterov) -> ()", &lars_update_op);
  m.def("lr_step(Tensor(a!) step, Tensor(b!) lr, float lr0, int warmup, int total, int mode) -> ()", &lr_step_op);
  m.def("augment(Tensor images, Tensor? indices, int n, int views, int OH, int OW, int Cpad, float strength, int seed, int counter, int view_offset, int flags, Tensor(a!) out, Tensor(b!)? params, int blur_kernel=0) -> ()", &augment_op);
  m.def("augment_max_blur_kernel() -> int", &augment_max_blur_kernel_op);
}
