// Host-side launchers of the simclr_amd gfx950 kernels (raw pointers + stream; no torch types,
// so the .hip translation units compile without the ATen headers).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

// Conv geometry for the implicit GEMM (see conv.hip / conv_hip.py for the derivations).
struct ConvGeom {
  int Nb, IH, IW, C;        // gathered input tensor NHWC (C % 8 == 0)
  int OH, OW;               // logical output grid (rows M = Nb*OH*OW)
  int KH, KW;               // taps
  int ish, isw, dh, dw;     // input = (oh*ish + kh*dh + ih0, ow*isw + kw*dw + iw0)
  int ih0, iw0;
  int N;                    // output channels (GEMM N)
  int OHp, OWp, osh, osw, ooh, oow, ldo;  // physical output mapping
};

// ---- conv.hip
// Optional fusions around the implicit GEMM (all pointers nullable / mode 0 = off).
struct ConvFusion {
  const float* pro_sc = nullptr;  // A/X-operand prologue: a = relu?(x*sc[seg][c] + sh[seg][c])
  const float* pro_sh = nullptr;
  int pro_seg_rows = 0;           // rows per segment (BM must divide it for igemm)
  int pro_relu = 0;
  int pro_S = 1;
  const float* pro_d = nullptr;   // igemm BN-backward prologue: a = sc·A + sh·A2 + d
  const uint16_t* A2 = nullptr;   //   second A-operand tensor (same geometry as A)
  const float* pro_rsc = nullptr; // igemm block-output prologue (pro_out != nullptr): a =
  const float* pro_rsh = nullptr; //   relu(A·sc + sh + A2·rsc + rsh), A2 = residual (rsc null:
  uint16_t* pro_out = nullptr;    //   identity), a and its ReLU bitmask stored to pro_out /
  uint8_t* pro_mask = nullptr;    //   pro_mask
  const uint16_t* dY2 = nullptr;  // wgrad dY-operand BN-backward prologue (coef [3][S][N])
  const float* dp_coef = nullptr;
  int dp_seg_rows = 0, dp_S = 1;
  int epi_mode = 0;               // igemm: 1 out = acc + a; 2 out = acc + (b > 0 ? a : 0);
  int epi_a_sub = 0;              // epi_a is the stride-2 subsampled [Nb][ceil(OH/2)][ceil(OW/2)][ldo]
                                  // tensor (a stride-2 1x1 downsample's compact dgrad): 0 at odd (oh, ow)
                                  // 3 out = (b*sc+sh > 0 ? acc : 0) + BN-bwd partials
                                  // 4 out = (b > 0 ? acc + a : 0) + BN-bwd partials vs c
  const uint16_t* epi_a = nullptr;
  const uint16_t* epi_b = nullptr;
  const uint16_t* epi_c = nullptr;  // mode 4: pre-BN activation for x̂
  const uint8_t* epi_mask = nullptr;  // mode 4: ReLU bitmask of the block input (see bn_apply_ss)
  const uint16_t* epi_c2 = nullptr;   // mode 4: second x̂ source (producer's downsample BN input)
  const float* epi_mi2 = nullptr;     //   and its mean/invstd [2][S][N]
  float* stats2 = nullptr;            //   partials Σg, Σg·x̂2 (layout of stats)
  const float* epi_ss = nullptr;  // mode 3: [2][S][N] scale/shift
  const float* epi_mi = nullptr;  // mode 3/4: [2][S][N] mean/invstd
  int epi_S = 1;
  int seg_rows = 0;               // rows per segment of the output (stats remap, mode 3)
  int stats_seg_blocks = 0;       // >0: segment-major stats rows (see conv.hip)
  int stats_base = 0;
};

int igemm_num_variants();
int igemm_variant_bm(int v);
int igemm_variant_bn(int v);
int igemm_default_variant(int N);
// What a tile variant is (kernel family, tile, waves, LDS stages, launcher) is one row of the
// descriptor tables in conv.hip; the predicates below read those rows.
bool igemm_variant_glds(int v);   // not the register-staged kernel: LDS-DMA or patch
bool igemm_variant_patch(int v);  // the LDS-resident-patch 3x3 kernel
bool igemm_glds_ok(const ConvGeom& g, bool pro, bool bn_bwd_pro);  // LDS-DMA geometry rule
bool igemm_patch_ok(const ConvGeom& g);                            // patch-kernel geometry rule
// Can tile variant v run this geometry with these operand prologues and this epilogue mode: the
// bindings' check, the launcher's check and the Python autotuner's candidate lists.  It is built
// on the set of (prologue, epilogue) pairs the launcher instantiates for the variant's family;
// of the epilogue it knows the one hole that depends on the tile (BN-backward prologue + mode 4
// on an LDS-DMA tile above 256 x 128), the others are fusion checks of the igemm binding.
bool igemm_variant_ok(int v, const ConvGeom& g, bool pro, bool bn_bwd_pro, int epi_mode = 0);
bool igemm_dual_ok(int v, const ConvGeom& g);  // ... with the block-output prologue
int igemm_block_m(int N);
void conv_igemm_nt(const ConvGeom& g, const uint16_t* A, size_t a_elems, const uint16_t* B,
                   uint16_t* out, const float* bias, float* stats, const ConvFusion& f,
                   int variant, hipStream_t s);
int wgrad_num_variants();
// wgrad_xp's step-affine X addressing: set the mode (>= 0) and/or return it (SIMCLR_WGRAD_XLIN)
int wgrad_xlin(int mode);
int wgrad_default_variant(int N);
bool wgrad_variant_glds(int v);  // LDS-DMA variant (see wgrad_variant_ok)
int wgrad_variant_area(int v);   // output tile elements (BCO x BKK)
bool wgrad_variant_ok(int v, const ConvGeom& g, bool pro, bool dy_pro);
int wgrad_splits(const ConvGeom& g, int variant);
void conv_wgrad(const ConvGeom& g, const uint16_t* dY, const uint16_t* X, size_t x_elems,
                float* partial, int splits, float* out, int Creal, float beta,
                const ConvFusion& f, int variant, hipStream_t s);
// fused 1x1 backward (dgrad + wgrad + BN2-backward partials in one pass, Co = 256, Ci = 64)
size_t conv1x1_bwd_dual_lds();
void conv1x1_bwd_dual(const uint16_t* G, const uint16_t* A3, const float* coef, const uint16_t* X,
                      const float* xss, const float* xmi, const uint16_t* Wt, uint16_t* gm,
                      float* stats, float* wpart, int M, int CO, int CI, int S, int bps,
                      hipStream_t s, const uint16_t* Xraw = nullptr, bool dual8 = false);
void conv1x1_bwd_dual_s2(const uint16_t* G, const uint16_t* A3, const float* coef,
                         const uint16_t* X, const uint16_t* Wt, uint16_t* gm, float* wpart,
                         int Mo, int CO, int CI, int S, int bps, int H, int W, int OH, int OW,
                         hipStream_t s);
void wgrad_reduce_slabs(float* partial, int splits, float* out, size_t n, float beta,
                        hipStream_t s);
// output tiles of a weight-gradient launch (ticket words of the in-kernel split reduction)
int wgrad_tiles(const ConvGeom& g, int variant);
// one dgrad weight transform (see weight_transform_batch): Wt[ci][khs][kws][co] =
// W[co][kh0 + khs*sh][kw0 + kws*sw][ci]; blocks [blk0, blk0 + nblk) of the batch launch
struct WtDesc {
  const uint16_t* W;
  uint16_t* Wt;
  int Co, KH, KW, Ci, KHs, KWs, kh0, sh, kw0, sw, blk0, nblk;
};
static_assert(sizeof(WtDesc) == 64, "WtDesc layout");
void conv_weight_transform_batch(const WtDesc* d, int n, int total_blocks, hipStream_t s);
void conv_weight_transform(const uint16_t* W, uint16_t* Wt, int Co, int KH, int KW, int Ci,
                           int KHs, int KWs, int kh0, int sh, int kw0, int sw, hipStream_t s);

// ---- bn.hip  (x: [R, C] bf16 rows, S segments of R/S rows each)
void bn_stats_partial(const uint16_t* x, int R, int C, int S, float* partial, int* nblk_per_seg,
                      hipStream_t s);
int bn_stats_blocks_per_seg(int R, int C, int S);
int bn_reduce_groups(int nblk);  // level-1 groups; workspace = S*groups*2*C floats
int bn_reduce_direct_rows();      // bn_reduce_fused: partials with <= this many rows per segment are
                                  // reduced by one block per channel group (no slices / ticket)
void bn_reduce_partials(const float* partial, int nblk_per_seg, int S, int C, float* stats,
                        float* ws, hipStream_t s);
void bn_finalize(const float* stats, int S, int C, float count, float eps, float momentum,
                 float* running_mean, float* running_var, float* mean_invstd, int64_t* nbt,
                 const float* gamma, const float* beta, float* scale_shift, hipStream_t s);
// One-launch reduce of [S][nblk][2][C] partials + (mode 0) stats out, (1) forward finalize,
// (2) backward finalize.  ws = S*groups*2*C floats; tickets = >= ceil(C/64) zeroed uints.
struct BnReduceFusedParams {
  const float* partial = nullptr;
  int nblk = 0, S = 1, C = 0, mode = 0;
  float* ws = nullptr;
  unsigned* tickets = nullptr;
  float* stats = nullptr;
  float count = 1.f, eps = 1e-5f, momentum = 0.1f;
  float* running_mean = nullptr;
  float* running_var = nullptr;
  float* mi = nullptr;
  int64_t* nbt = nullptr;
  const float* gamma = nullptr;
  const float* beta = nullptr;
  float* ss = nullptr;
  float* dgamma = nullptr;
  float* dbeta = nullptr;
  float* coef = nullptr;
  // cross-rank exchange over IPC-mapped peer arenas (modes 1 / 2 at world > 1, see bn.hip)
  uint64_t* const* ipc_peers = nullptr;  // device array [world] of arena bases (own included)
  uint64_t* ipc_own = nullptr;           // this rank's arena base
  long long ipc_site = 0;                // word offset of this BatchNorm's region
  unsigned* ipc_epoch = nullptr;         // [ceil(C/64)] per-site exchange counters
  int* ipc_err = nullptr;                // set on a spin timeout
  int world = 1, rank = 0;
};
void bn_reduce_fused(const BnReduceFusedParams& q, hipStream_t s);
// words of one exchange region: 2 parities x world x [2][S][C] (LL words: value | epoch << 32)
inline long long bn_ipc_region_words(int world, int S, int C) {
  return 2LL * world * 2 * S * C;
}

// ---- comm.hip: one-shot IPC all-gather (op 0) / reduce-scatter (op 1) of 32-bit words over the
// peer-mapped arenas (LL words; site = 2 parities x world x n words, IPC_COLL_BLOCKS epoch
// counters)
constexpr int IPC_COLL_BLOCKS = 64;
long long ipc_coll_region_words(int world, int n);
void ipc_collective(int op, const uint32_t* src, uint32_t* dst, int n, uint64_t* const* peers,
                    uint64_t* own, long long site, unsigned* epoch, int* err, int world,
                    int rank, hipStream_t s);
// y = relu?(x*sc + sh + [res | res*rsc + rsh]); ss / rss are [2][S][C] scale/shift tables
// optional mask: uint8 [R][C/8], bit e of byte (r, c/8) = (y[r][c] > 0)
void bn_apply_ss(const uint16_t* x, const float* ss, const uint16_t* res, const float* rss,
                 uint16_t* y, uint8_t* mask, int R, int C, int S, int relu, hipStream_t s);
void bn_apply(const uint16_t* x, const uint16_t* res, uint16_t* y, const float* mean_invstd,
              const float* gamma, const float* beta, int R, int C, int S, int relu,
              hipStream_t s);
void bn_apply_eval(const uint16_t* x, const uint16_t* res, uint16_t* y, const float* rmean,
                   const float* rvar, const float* gamma, const float* beta, float eps, int R,
                   int C, int relu, hipStream_t s);
void bn_bwd_reduce(const uint16_t* dy, const uint16_t* y, const uint16_t* x,
                   const float* mean_invstd, int R, int C, int S, int relu, float* partial,
                   hipStream_t s);
void bn_bwd_finalize(const float* sums, const float* mean_invstd, const float* gamma, int S, int C,
                     float count, float* dgamma, float* dbeta, float* coef, hipStream_t s);
void bn_bwd_apply(const uint16_t* dy, const uint16_t* y, const uint16_t* x, const float* coef,
                  int R, int C, int S, int relu, uint16_t* dx, uint16_t* dres, hipStream_t s);
// two BatchNorms fed by the same gradient (residual block: last BN + downsample BN):
// dx1 = A1·g + B1·x1 + D1, dx2 = A2·g + B2·x2 + D2 in one pass over g
void bn_bwd_apply2(const uint16_t* g, const uint16_t* x1, const float* coef1, uint16_t* dx1,
                   const uint16_t* x2, const float* coef2, uint16_t* dx2, int R, int C, int S,
                   hipStream_t s);

// ---- misc.hip
void avgpool_fwd(const uint16_t* x, uint16_t* y, int Nb, int HW, int C, hipStream_t s);
void avgpool_bwd(const uint16_t* dy, uint16_t* dx, int Nb, int HW, int C, hipStream_t s);
int colsum_groups(int R);  // workspace = colsum_groups(R) * C floats
// split-K GEMM for small M: out = f(A)·Bᵀ (+ bias), f = BN + ReLU per (row segment, column)
// when sc != nullptr; part = [KS][M][N] fp32 scratch (misc.hip)
void gemm_sk(const uint16_t* A, const uint16_t* B, const float* sc, const float* sh, int seg,
             int M, int N, int K, int KS, float* part, const float* bias, uint16_t* out,
             hipStream_t s);
void colsum_bf16(const uint16_t* x, int R, int C, float* out, float beta, float* ws,
                 hipStream_t s);
void cast_f32_bf16(const float* x, uint16_t* y, size_t n, hipStream_t s);
void cast_bf16_f32(const uint16_t* x, float* y, size_t n, hipStream_t s);

// ---- ntxent.hip  (exact fp32 on v_mfma_f32_16x16x4_f32)
void ntxent_normalize_f32(const uint16_t* z, int R, int D, float* zn, float* inv_norm,
                          hipStream_t s);
void ntxent_transpose(const float* in, float* out, int R, int D, hipStream_t s);
// in [R][D] -> columns [c0, c0 + R) of out [D][ldo]
void ntxent_transpose_cols(const float* in, float* out, int R, int D, int ldo, int c0,
                           hipStream_t s);
// forward partials of the columns [c_lo, c_hi) into splits [split_base, +splits), and the merge
void ntxent_forward_range(const float* znT, int R, int Ccols, int D, int col_offset, int n_local,
                          float inv_temp, float* part, int c_lo, int c_hi, int splits,
                          int split_base, hipStream_t s);
void ntxent_finish(const float* part, int R, int splits, float* lse, float* loss, hipStream_t s);
int ntxent_fwd_splits(int R, int Ccols);
int ntxent_bwd_splits(int nown, int npart);
void ntxent_forward(const float* znT, int R, int Ccols, int D, int col_offset, int n_local,
                    float inv_temp, float* part, int splits, float* lse, float* loss,
                    hipStream_t s);
void ntxent_backward_part(int row_mode, const float* zn, const float* znT, const float* lse, int R,
                          int Ccols, int D, int col_offset, int n_local, float inv_temp,
                          float gscale, const float* gout, float* part, int splits, float* out,
                          hipStream_t s);
void ntxent_normalize_backward(const float* zn, const float* inv_norm, const float* dzn, int R,
                               int D, uint16_t* dz_bf16, float* dz_f32, hipStream_t s);
void ntxent_reduce_loss(const float* loss_rows, int R, float scale, float* out, hipStream_t s);
// label mode (SupCon): positives = the columns with the anchor's label.  ycol: int32 labels of
// the columns [y0, ...) (forward) / of every column (backward); part holds 4 floats per row
void supcon_forward_range(const float* znT, const int* ycol, int y0, int R, int Ccols, int D,
                          int col_offset, float inv_temp, float* part, int c_lo, int c_hi,
                          int splits, int split_base, hipStream_t s);
void supcon_finish(const float* part, int R, int splits, float* lse, float* inv_cnt, float* loss,
                   hipStream_t s);
void supcon_backward_part(int row_mode, const float* zn, const float* znT, const float* lse,
                          const float* inv_cnt, const int* ycol, int R, int Ccols, int D,
                          int col_offset, float inv_temp, float gscale, const float* gout,
                          float* part, int splits, float* out, hipStream_t s);
// weighted negatives (hard-negative beta >= 0, debiased 0 <= tau_plus < 1, decoupled): the
// positive leaves the sums; part holds 5 floats per row if beta > 0, else 3; stats [R][4] =
// (L1, A, B, L0) per row, written by the finish and read by the backward passes
void ntxent_weighted_forward_range(const float* znT, int R, int Ccols, int D, int col_offset,
                                   int n_local, float inv_temp, float beta, float* part, int c_lo,
                                   int c_hi, int splits, int split_base, hipStream_t s);
void ntxent_weighted_finish(const float* part, int R, int splits, int Ccols, float inv_temp,
                            float beta, float tau_plus, int decoupled, float* stats, float* loss,
                            hipStream_t s);
void ntxent_weighted_backward_part(int row_mode, const float* zn, const float* znT,
                                   const float* stats, int R, int Ccols, int D, int col_offset,
                                   int n_local, float inv_temp, float beta, float gscale,
                                   const float* gout, float* part, int splits, float* out,
                                   hipStream_t s);
// out[v*n + i] = labels[idx ? idx[i] : i] (int32 or int64 labels, n_src of them), v < views
void supcon_expand_labels(const void* labels, int labels_i64, const int64_t* idx, long n_src,
                          int n, int views, int* out, hipStream_t s);

// ---- barlow.hip  (Barlow Twins: cross-correlation over the batch on v_mfma_f32_16x16x32_bf16)
// n % 32 == 0, D % 64 == 0, 64 <= D <= 2048.  z [2n][D] (bf16, or fp32 with z_f32) ->
// rstd [2][D], zh bf16 [2n][D], zhT bf16 [2][D][n]
void barlow_standardize(const void* z, int z_f32, int n, int D, float eps, float* rstd,
                        uint16_t* zh, uint16_t* zhT, hipStream_t s);
int barlow_corr_splits(int n, int D);
// part [splits][D][D]: the correlation over slices of the batch (unscaled)
void barlow_corr(const uint16_t* zhT, int n, int D, int splits, float* part, hipStream_t s);
int barlow_loss_blocks(int D);
// C [D][D] = (Σ part) / n, lpart[barlow_loss_blocks(D)] = partial sums of the loss terms
void barlow_loss(const float* part, int splits, int n, int D, float lambd, float* C, float* lpart,
                 hipStream_t s);
// G, GT bf16 [D][D] from C and the upstream scalar gout[0]
void barlow_grad(const float* C, int D, float lambd, const float* gout, uint16_t* G, uint16_t* GT,
                 hipStream_t s);
// dzh fp32 [2n][D], colpart [2][n/32][2][D] (per row tile: column sums of dzh and of dzh·zh)
void barlow_backward(const uint16_t* zh, const uint16_t* G, const uint16_t* GT, int n, int D,
                     float* dzh, float* colpart, hipStream_t s);
// dz (bf16 or fp32, the other null) from dzh and the column means: colpart's tiles added in order, / n
void barlow_std_backward(const uint16_t* zh, const float* rstd, const float* dzh,
                         const float* colpart, int n, int D, uint16_t* dz_bf16, float* dz_f32,
                         hipStream_t s);
// the loss over W ranks of n rows each (loss.barlow_global), around three collectives:
// stats [2][2][D] = (μ_r, M2_r) per view; gstats [W][2][2][D] the all-gathered ones, merged in
// rank order into rstd, zh, zhT; S [D][D] = Σ part in split order (undivided, to be all-reduced);
// csum [2][2][D] = colpart summed in tile order; gsum [W][2][2][D] the all-gathered ones, which
// barlow_std_backward_global (the kernel of barlow_std_backward) adds in rank order, / (W·n)
void barlow_stats(const void* z, int z_f32, int n, int D, float* stats, hipStream_t s);
void barlow_merge_standardize(const void* z, int z_f32, const float* gstats, int W, int n, int D,
                              float eps, float* rstd, uint16_t* zh, uint16_t* zhT, hipStream_t s);
void barlow_slab_merge(const float* part, int splits, int D, float* S, hipStream_t s);
void barlow_colsum(const float* colpart, int n, int D, float* csum, hipStream_t s);
void barlow_std_backward_global(const uint16_t* zh, const float* rstd, const float* dzh,
                                const float* gsum, int W, int n, int D, uint16_t* dz_bf16,
                                float* dz_f32, hipStream_t s);

// ---- nnclr.hip  (NNCLR: nearest-neighbour lookup in a FIFO support set, cross-view InfoNCE)
int nnclr_top1_splits(int R, int Q);  // queue splits of the lookup
int nnclr_loss_splits(int n);         // column / anchor splits of the loss forward / backward
// z [R][D] bf16 or fp32 -> zn fp32, zb bf16 (ẑ rounded once), inv_norm [R]
void nnclr_normalize(const void* z, int z_f32, int R, int D, float* zn, uint16_t* zb,
                     float* inv_norm, hipStream_t s);
// idx[r] = argmax_k zb_r · Qm_k (similarity descending, index ascending), a[r] = Qm[idx[r]];
// candv / candi [splits][R] scratch.  R % 32 == 0, Q % 64 == 0, D in {32, 64, 128, 256}
void nnclr_lookup(const uint16_t* zb, const uint16_t* Qm, int R, int Q, int D, int splits,
                  float* candv, int* candi, int* idx, uint16_t* a, hipStream_t s);
// part [splits][2n][3] in ntxent_finish's format
void nnclr_forward(const uint16_t* a, const uint16_t* zb, int n, int D, float inv_temp, int splits,
                   float* part, hipStream_t s);
// part [splits][2n][D] scratch; dz in bf16 or fp32 (one of the two)
void nnclr_backward(const uint16_t* a, const uint16_t* zb, const float* zn, const float* inv_norm,
                    const float* lse, int n, int D, float inv_temp, const float* gout, int splits,
                    float* part, uint16_t* dz_bf16, float* dz_f32, hipStream_t s);
// rows [0, n) of zb -> Qm[(cursor + b) mod Q], cursor <- (cursor + n) mod Q (one launch)
void nnclr_enqueue(const uint16_t* zb, int n, int D, int Q, uint16_t* Qm, int* cursor,
                   hipStream_t s);

// ---- lars.hip (flat fp32 master / grad / momentum, bf16 shadow; per-segment table)
void lars_norms(const float* p, const float* g, const int* chunk_beg, const int* chunk_end,
                int nchunks, float grad_scale, float* norms, hipStream_t s);
void lars_update(float* p, const float* g, float* mom, uint16_t* shadow, const int* chunk_seg,
                 const int* chunk_beg, const int* chunk_end, int nchunks, const int* seg_chunk_beg,
                 const int* seg_chunk_end, const float* seg_wd, const int* seg_flags,
                 const float* norms, const float* lr_ptr, float momentum, float trust, float eps,
                 float grad_scale, int nesterov, hipStream_t s);
void lr_schedule_step(int64_t* step, float* lr_out, double lr0, int64_t warmup, int64_t total,
                      int mode, hipStream_t s);

// ---- augment.hip
void simclr_augment(const uint8_t* images, const int64_t* indices, int n, int views, int H, int W,
                    int OH, int OW, int Cpad, float strength, uint64_t seed, uint64_t counter,
                    int view_offset, int flags, uint16_t* out, float* params_out, int blur_kernel,
                    hipStream_t s);
int augment_max_blur_kernel();  // blur_kernel: 0 (off) or odd in [3, this]
// output rows per LDS band of a blurred image; 0: (OH, OW, ks) cannot be blurred
int augment_blur_band(int OH, int OW, int ks);

// ---- eval.hip: maxpool (K2), cross-entropy + top-k (K10), centroid class sums (K11)
void maxpool_fwd(const uint16_t* x, uint16_t* y, uint8_t* arg, int Nb, int H, int W, int C,
                 int OH, int OW, int K, int S, int P, hipStream_t s);
void maxpool_bwd(const uint16_t* dy, const uint8_t* arg, uint16_t* dx, int Nb, int H, int W,
                 int C, int OH, int OW, int K, int S, int P, hipStream_t s);
// ImageNet stem as a 4x4 stride-1 conv: 2x2 space-to-depth of the P-padded image (C <= 4 real)
void stem_s2d(const uint16_t* img, uint16_t* xs, int Nb, int H, int W, int Cin, int creal,
              int HS, int WS, int P, hipStream_t s);
void bn_relu_maxpool(const uint16_t* a, const float* ss, int S, uint16_t* y, uint8_t* arg,
                     uint16_t* asel, int Nb, int H, int W, int C, int OH, int OW, int K, int Sd,
                     int P, hipStream_t s);
void maxpool_bwd_bn(const uint16_t* gy, const uint8_t* arg, const uint16_t* y, const uint16_t* a,
                    const float* coef, int S, uint16_t* da, int Nb, int H, int W, int C, int OH,
                    int OW, int K, int Sd, int P, hipStream_t s);
void ce_topk(const float* logits, const int64_t* y, int B, int C, float gscale, float* loss,
             int* rank, float* dlogits, hipStream_t s);
size_t class_sums_lds(int NC);
int class_sums_groups(int N);
void class_sums(const float* X, const int64_t* y, int N, int D, int NC, float* part, float* pcnt,
                float* sums, float* counts, hipStream_t s);


// ---- knn.hip: weighted k-NN probe (normalise + round, fused similarity / top-k, class vote)
int knn_kstep();        // Dp is D rounded up to this
int knn_max_k();
int knn_max_classes();
size_t knn_topk_lds();  // bytes of LDS of the top-k kernel
int knn_splits(int Q, int N);
size_t knn_buf_keys(int Q, int N);          // 8-byte keys of append-buffer scratch
size_t knn_cand_keys(int Q, int N, int k);  // 8-byte keys of per-split candidates
void knn_normalize(const void* x, bool x_is_bf16, int R, int D, int Dp, uint16_t* out,
                   hipStream_t s);
void knn_topk(const uint16_t* Qn, const uint16_t* Bn, int Q, int N, int Dp, int k, bool has_self,
              long long self_off, unsigned long long* buf, unsigned long long* cand, float* vals,
              int* idx, hipStream_t s);
void knn_vote(const float* vals, const int* idx, const int64_t* labels, const int64_t* targets,
              int Q, int k, int N, int C, float inv_t, float* scores, int* rank, hipStream_t s);

// ---- kmeans.hip: spherical k-means probe (R restarts in the same launches: fused similarity /
// top-1 assignment, one-hot GEMM centroid update, slab merge + normalise)
int km_kstep();         // Fp is F rounded up to this
int km_max_restarts();  // R
int km_max_cols();      // R * Kp
int km_max_fp();
int km_splits(int N, int Fp);                    // row splits of the update: independent of R
size_t km_slab_floats(int N, int Fp, int RK);    // fp32 scratch of the update
// X [N][Fp], C [R * Kp][Fp] bf16; a [R][N] (read as the previous assignment, then overwritten),
// s [R][N]; counts [R * Kp] += rows per cluster; changed [R][Tp1], column *it += changed rows
void km_assign(const uint16_t* X, const uint16_t* C, int N, int Fp, int K, int Kp, int R, int* a,
               float* s, int* counts, int* changed, const int* it, int Tp1, hipStream_t st);
// C <- normalised sums of the rows assigned by a (S [R * Kp][Fp], optional: the merged sums);
// clears counts, *it += 1
void km_update(const uint16_t* X, const int* a, int N, int Fp, int K, int Kp, int R, int* counts,
               uint16_t* C, float* S, float* slab, int* it, hipStream_t st);
void km_objective(const float* s, int R, int N, double* J, hipStream_t st);

// ---- geometry.hip: geometry probe (pair statistics of the Gram matrix's upper triangle consumed
// in registers; centred features, their second-moment matrix by its upper triangle)
int geo_kstep();       // Dp is D rounded up to this
int geo_max_dp();
int geo_chunk();       // rows per fp32 accumulation chunk of the second-moment product
int geo_pair_chain();  // the longest fp32 chain of roundings in a pair tile's sums
long long geo_pair_tiles(int N);      // 128 x 128 tiles on or above the diagonal
int geo_syrk_tiles(int Dp);           // 64 x 64 tiles on or above the diagonal
int geo_syrk_splits(int N, int Dp);   // splits of the chunks over blocks
// Xn [N][Dp] bf16, labels [N] or null; fpart [tiles][3] = (E, A, A_same), ipart [tiles][2] =
// (pairs, same pairs) per tile; c2t = 2 t
void geo_pair(const uint16_t* Xn, const int* labels, int N, int Dp, float c2t, float* fpart,
              int* ipart, hipStream_t s);
// x [N][D] fp32 -> mu [Dp], cT [Dp][Np] bf16 (Np = N rounded up to 64); csum [chunks][Dp] scratch
void geo_center(const float* x, int N, int D, int Dp, int Np, double* csum, float* mu,
                uint16_t* cT, hipStream_t s);
// S [Dp][Dp] fp64 = c^T c; slab [splits][tiles][64][64] fp64 scratch
void geo_syrk(const uint16_t* cT, int N, int Dp, int Np, double* slab, double* S, hipStream_t s);

// ---- probe.hip: linear-probe sweep (G classifiers on one feature batch: fused forward / CE /
// gradient, fused weight gradient / Nesterov SGD update)
int probe_kstep();        // Fp is F rounded up to this
int probe_max_configs();  // G
int probe_max_cols();     // G * Cp
int probe_max_rows();     // rows of one call
struct ProbeFwdArgs {
  const uint16_t* X;      // [N][Fp] bf16 features
  const int64_t* y;       // [N] labels
  const int64_t* idx;     // [rows] gathered feature rows
  long long N;
  int Fp, rows, Rp;       // Rp: rows rounded up to 32 (training) or 16 (evaluation)
  int G, C, Cp;
  const uint16_t* Wsh;    // [G * Cp][Fp] bf16 shadow weights
  const float* bias;      // [G * Cp]
  float* Z;               // [>= rows][G * Cp] logits scratch
  float* loss;            // loss[g * loss_stride + row]
  long long loss_stride;
  int* rank;              // [G][rows] or null
  uint16_t* dlT;          // [G * Cp][ldr] bf16 or null (evaluation)
  int ldr;
  float* dbp;             // [ceil(rows / 16)][G * Cp] bias-gradient partials
};
void probe_forward(const ProbeFwdArgs& a, hipStream_t s);
struct ProbeUpdArgs {
  const uint16_t* X;
  const int64_t* idx;
  long long N;
  int Fp, rows, Rp, G, C, Cp;
  const uint16_t* dlT;
  int ldr;
  const float* dbp;
  float *W, *Mw, *b, *Mb;  // fp32 master and momentum
  uint16_t* Wsh;
  const float *lr0, *wd;   // [G]
  const float* ftab;       // cosine factors per step
  int step;
  float momentum;
};
void probe_update(const ProbeUpdArgs& a, hipStream_t s);

// ---- probe.hip, online probe: one linear classifier trained on the encoder output inside the
// captured pre-training step, on the sweep's forward and weight-gradient kernels under its own
// row policy; whatever changes per step is read from device memory
int online_probe_kstep();     // Fp is F rounded up to this
int online_probe_max_cols();  // Cp
int online_probe_max_fp();
int online_probe_max_rows();
struct OnlineProbeFwdArgs {
  const uint16_t* X;    // [rows][Fp] bf16 encoder output, both views
  const int* y;         // [n] labels: row r has y[r % n]
  int n, rows, Rp;      // rows % 16 == 0; Rp: rows rounded up to 32
  int Fp, C, Cp;
  const uint16_t* Wsh;  // [Cp][Fp] bf16 shadow weights
  const float* bias;    // [Cp]
  float* Z;             // [rows][Cp] logits scratch
  float* loss;          // [rows]
  int* rank;            // [rows]
  uint16_t* dlT;        // [Cp][Rp] bf16
  float* dbp;           // [rows / 16][Cp] bias-gradient partials
};
void online_probe_forward(const OnlineProbeFwdArgs& a, hipStream_t s);
// acc_loss [1] += sum of loss; acc_cnt [3] += (rank == 0, rank < top_k, rows)
void online_probe_metrics(const float* loss, const int* rank, int rows, int top_k,
                          double* acc_loss, long long* acc_cnt, hipStream_t s);
struct OnlineProbeGradArgs {
  const uint16_t* X;
  int rows, Rp, Fp, Cp;
  const uint16_t* dlT;
  const float* dbp;
  float* grad;          // [Cp * Fp + Cp]: dW then db
};
void online_probe_wgrad(const OnlineProbeGradArgs& a, hipStream_t s);
struct OnlineProbeUpdArgs {
  float *master, *mom;  // [Cp * Fp + Cp]
  const float* grad;
  uint16_t* shadow;     // [Cp * Fp]
  const float* lr;      // [1] the probe's LR cell (lr_step)
  float wd, momentum, gscale;
  int C, Cp, F, Fp;
};
void online_probe_update(const OnlineProbeUpdArgs& a, hipStream_t s);
