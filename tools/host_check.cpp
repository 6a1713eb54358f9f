// Host-side invariants of the kernel launchers, built with AddressSanitizer + UBSan by
// tests/test_host_sanitizers.py (sanitizer builds of the C++ host code; GPU-side
// sanitizers are unavailable on this pool).  Only host logic runs here — the tile-variant
// admissibility / split planning of conv.hip, the BatchNorm reduction planning of bn.hip and
// the split / workspace arithmetic of ntxent.hip and eval.hip — over every convolution of
// ResNet-18/50 at the CIFAR (32x32) and ImageNet (224x224) shapes, in all three passes.
//
// --dump prints the conv tile-variant tables and the admissibility / split planning of a fixed
// geometry list as JSON rows, using only the API that tests/golden/conv_variant_table_v1.json was
// recorded with (this file built with -DHOST_CHECK_V1_API against the tree before the variant
// descriptor tables); tests/test_host_sanitizers.py compares the two row for row.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../simclr_amd/csrc/kernels.h"

namespace {

int failures = 0;
#define EXPECT(cond, ...)                                  \
  do {                                                     \
    if (!(cond)) {                                         \
      std::fprintf(stderr, "FAIL %s: ", #cond);            \
      std::fprintf(stderr, __VA_ARGS__);                   \
      std::fprintf(stderr, "\n");                          \
      ++failures;                                          \
    }                                                      \
  } while (0)

ConvGeom fwd_geom(int N, int H, int W, int C, int k, int s, int p, int Co) {
  const int OH = (H + 2 * p - k) / s + 1, OW = (W + 2 * p - k) / s + 1;
  return ConvGeom{N, H, W, C, OH, OW, k, k, s, s, 1, 1, -p, -p, Co, OH, OW, 1, 1, 0, 0, Co};
}

struct Conv { int C, Co, k, s, H; };

std::vector<Conv> resnet_convs(bool bottleneck, int H0, bool imagenet_stem) {
  std::vector<Conv> v;
  int H = H0;
  if (imagenet_stem) { v.push_back({8, 64, 7, 2, H}); H = (H + 6 - 7) / 2 + 1; H = (H + 2 - 3) / 2 + 1; }
  else v.push_back({8, 64, 3, 1, H});
  int inpl = 64;
  const int planes[4] = {64, 128, 256, 512}, blocks[4] = {bottleneck ? 3 : 2, bottleneck ? 4 : 2,
                                                          bottleneck ? 6 : 2, bottleneck ? 3 : 2};
  for (int l = 0; l < 4; ++l) {
    for (int b = 0; b < blocks[l]; ++b) {
      const int s = (b == 0 && l > 0) ? 2 : 1;
      const int out = bottleneck ? planes[l] * 4 : planes[l];
      if (bottleneck) {
        v.push_back({inpl, planes[l], 1, 1, H});
        v.push_back({planes[l], planes[l], 3, s, H});
        const int Ho = (H + 2 - 3) / s + 1;
        v.push_back({planes[l], out, 1, 1, Ho});
      } else {
        v.push_back({inpl, planes[l], 3, s, H});
        const int Ho = (H + 2 - 3) / s + 1;
        v.push_back({planes[l], planes[l], 3, 1, Ho});
      }
      if (b == 0 && (s != 1 || inpl != out)) v.push_back({inpl, out, 1, s, H});
      H = (H + 2 - 3) / s + 1;
      inpl = out;
    }
  }
  return v;
}

void check_net(const char* name, bool bottleneck, int H0, bool imagenet, int batch) {
  for (const Conv& c : resnet_convs(bottleneck, H0, imagenet)) {
    const int p = c.k / 2;
    const ConvGeom g = fwd_geom(batch, c.H, c.H, c.C, c.k, c.s, p, c.Co);
    const long long M = (long long)g.Nb * g.OH * g.OW;
    int ok = 0;
    for (int v = 0; v < igemm_num_variants(); ++v) {
      const int bm = igemm_variant_bm(v), bn = igemm_variant_bn(v);
      EXPECT(bm > 0 && bn > 0 && bm % 16 == 0 && bn % 16 == 0, "%s variant %d tile %dx%d", name, v,
             bm, bn);
      ok += igemm_variant_ok(v, g, false, false) ? 1 : 0;
      (void)igemm_dual_ok(v, g);
    }
    EXPECT(ok > 0, "%s: no igemm variant for C=%d Co=%d k=%d s=%d H=%d", name, c.C, c.Co, c.k, c.s, c.H);
    int wok = 0;
    for (int v = 0; v < wgrad_num_variants(); ++v) {
      if (!wgrad_variant_ok(v, g, false, false)) continue;
      ++wok;
      const int sp = wgrad_splits(g, v);
      EXPECT(sp >= 1 && (long long)sp <= (M + 63) / 64, "%s wgrad splits %d for M=%lld", name, sp, M);
    }
    EXPECT(wok > 0 || c.C % 8 != 0, "%s: no wgrad variant for C=%d Co=%d k=%d", name, c.C, c.Co, c.k);
    const int nb = bn_stats_blocks_per_seg((int)(M / 2), c.Co, 2);
    EXPECT(nb >= 1, "%s bn blocks", name);
    const int G = bn_reduce_groups(nb);
    EXPECT(G >= 1 && G <= nb, "%s bn groups %d of %d rows", name, G, nb);
    EXPECT(bn_ipc_region_words(8, 2, c.Co) == 2LL * 8 * 2 * 2 * c.Co, "%s ipc region", name);
  }
}

// The geometries of the dump: every pinned shape of bench/tiles_mi355x.json, the parametrisations
// of tests/test_gpu_kernels.py, and a few that the LDS-DMA / patch kernels must reject.
const ConvGeom DUMP_GEOMS[] = {
    // pinned tile
    {1024, 1, 1, 128, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 2048, 1, 1, 1, 1, 0, 0, 2048},
    {1024, 1, 1, 2048, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 128, 1, 1, 1, 1, 0, 0, 128},
    {1024, 1, 1, 2048, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 2048, 1, 1, 1, 1, 0, 0, 2048},
    {1024, 16, 16, 128, 16, 16, 1, 1, 1, 1, -1, -1, 0, 0, 128, 32, 32, 2, 2, 0, 0, 128},
    {1024, 16, 16, 128, 16, 16, 1, 1, 1, 1, 1, 1, 0, 0, 512, 16, 16, 1, 1, 0, 0, 512},
    {1024, 16, 16, 128, 16, 16, 1, 2, 1, 1, -1, -1, 0, 1, 128, 32, 32, 2, 2, 0, 1, 128},
    {1024, 16, 16, 128, 16, 16, 2, 1, 1, 1, -1, -1, 1, 0, 128, 32, 32, 2, 2, 1, 0, 128},
    {1024, 16, 16, 128, 16, 16, 2, 2, 1, 1, -1, -1, 1, 1, 128, 32, 32, 2, 2, 1, 1, 128},
    {1024, 16, 16, 128, 16, 16, 3, 3, 1, 1, 1, 1, -1, -1, 128, 16, 16, 1, 1, 0, 0, 128},
    {1024, 16, 16, 256, 16, 16, 1, 1, 1, 1, 1, 1, 0, 0, 512, 16, 16, 1, 1, 0, 0, 512},
    {1024, 16, 16, 256, 8, 8, 3, 3, 2, 2, 1, 1, -1, -1, 256, 8, 8, 1, 1, 0, 0, 256},
    {1024, 16, 16, 512, 16, 16, 1, 1, 1, 1, 1, 1, 0, 0, 128, 16, 16, 1, 1, 0, 0, 128},
    {1024, 16, 16, 512, 16, 16, 1, 1, 1, 1, 1, 1, 0, 0, 256, 16, 16, 1, 1, 0, 0, 256},
    {1024, 16, 16, 512, 8, 8, 1, 1, 2, 2, 1, 1, 0, 0, 1024, 8, 8, 1, 1, 0, 0, 1024},
    {1024, 32, 32, 128, 16, 16, 3, 3, 2, 2, 1, 1, -1, -1, 128, 16, 16, 1, 1, 0, 0, 128},
    {1024, 32, 32, 128, 32, 32, 1, 1, 1, 1, 1, 1, 0, 0, 256, 32, 32, 1, 1, 0, 0, 256},
    {1024, 32, 32, 256, 16, 16, 1, 1, 2, 2, 1, 1, 0, 0, 512, 16, 16, 1, 1, 0, 0, 512},
    {1024, 32, 32, 256, 32, 32, 1, 1, 1, 1, 1, 1, 0, 0, 128, 32, 32, 1, 1, 0, 0, 128},
    {1024, 32, 32, 256, 32, 32, 1, 1, 1, 1, 1, 1, 0, 0, 64, 32, 32, 1, 1, 0, 0, 64},
    {1024, 32, 32, 64, 32, 32, 1, 1, 1, 1, 1, 1, 0, 0, 256, 32, 32, 1, 1, 0, 0, 256},
    {1024, 32, 32, 64, 32, 32, 1, 1, 1, 1, 1, 1, 0, 0, 64, 32, 32, 1, 1, 0, 0, 64},
    {1024, 32, 32, 64, 32, 32, 3, 3, 1, 1, 1, 1, -1, -1, 64, 32, 32, 1, 1, 0, 0, 64},
    {1024, 32, 32, 8, 32, 32, 3, 3, 1, 1, 1, 1, -1, -1, 64, 32, 32, 1, 1, 0, 0, 64},
    {1024, 4, 4, 2048, 4, 4, 1, 1, 1, 1, 1, 1, 0, 0, 1024, 4, 4, 1, 1, 0, 0, 1024},
    {1024, 4, 4, 2048, 4, 4, 1, 1, 1, 1, 1, 1, 0, 0, 512, 4, 4, 1, 1, 0, 0, 512},
    {1024, 4, 4, 512, 4, 4, 1, 1, 1, 1, -1, -1, 0, 0, 512, 8, 8, 2, 2, 0, 0, 512},
    {1024, 4, 4, 512, 4, 4, 1, 1, 1, 1, 1, 1, 0, 0, 2048, 4, 4, 1, 1, 0, 0, 2048},
    {1024, 4, 4, 512, 4, 4, 1, 2, 1, 1, -1, -1, 0, 1, 512, 8, 8, 2, 2, 0, 1, 512},
    {1024, 4, 4, 512, 4, 4, 2, 1, 1, 1, -1, -1, 1, 0, 512, 8, 8, 2, 2, 1, 0, 512},
    {1024, 4, 4, 512, 4, 4, 2, 2, 1, 1, -1, -1, 1, 1, 512, 8, 8, 2, 2, 1, 1, 512},
    {1024, 4, 4, 512, 4, 4, 3, 3, 1, 1, 1, 1, -1, -1, 512, 4, 4, 1, 1, 0, 0, 512},
    {1024, 8, 8, 1024, 4, 4, 1, 1, 2, 2, 1, 1, 0, 0, 2048, 4, 4, 1, 1, 0, 0, 2048},
    {1024, 8, 8, 1024, 8, 8, 1, 1, 1, 1, 1, 1, 0, 0, 256, 8, 8, 1, 1, 0, 0, 256},
    {1024, 8, 8, 1024, 8, 8, 1, 1, 1, 1, 1, 1, 0, 0, 512, 8, 8, 1, 1, 0, 0, 512},
    {1024, 8, 8, 256, 8, 8, 1, 1, 1, 1, -1, -1, 0, 0, 256, 16, 16, 2, 2, 0, 0, 256},
    {1024, 8, 8, 256, 8, 8, 1, 1, 1, 1, 1, 1, 0, 0, 1024, 8, 8, 1, 1, 0, 0, 1024},
    {1024, 8, 8, 256, 8, 8, 1, 2, 1, 1, -1, -1, 0, 1, 256, 16, 16, 2, 2, 0, 1, 256},
    {1024, 8, 8, 256, 8, 8, 2, 1, 1, 1, -1, -1, 1, 0, 256, 16, 16, 2, 2, 1, 0, 256},
    {1024, 8, 8, 256, 8, 8, 2, 2, 1, 1, -1, -1, 1, 1, 256, 16, 16, 2, 2, 1, 1, 256},
    {1024, 8, 8, 256, 8, 8, 3, 3, 1, 1, 1, 1, -1, -1, 256, 8, 8, 1, 1, 0, 0, 256},
    {1024, 8, 8, 512, 4, 4, 3, 3, 2, 2, 1, 1, -1, -1, 512, 4, 4, 1, 1, 0, 0, 512},
    {1024, 8, 8, 512, 8, 8, 1, 1, 1, 1, 1, 1, 0, 0, 1024, 8, 8, 1, 1, 0, 0, 1024},
    // test_conv_fwd_dgrad_wgrad
    {4, 8, 8, 64, 8, 8, 3, 3, 1, 1, 1, 1, -1, -1, 64, 8, 8, 1, 1, 0, 0, 64},
    {3, 9, 9, 64, 5, 5, 3, 3, 2, 2, 1, 1, -1, -1, 128, 5, 5, 1, 1, 0, 0, 128},
    {2, 8, 8, 128, 8, 8, 1, 1, 1, 1, 1, 1, 0, 0, 256, 8, 8, 1, 1, 0, 0, 256},
    {2, 8, 8, 256, 4, 4, 1, 1, 2, 2, 1, 1, 0, 0, 512, 4, 4, 1, 1, 0, 0, 512},
    {5, 8, 8, 8, 12, 12, 3, 3, 1, 1, 1, 1, -3, -3, 64, 12, 12, 1, 1, 0, 0, 64},
    {2, 16, 16, 8, 8, 8, 7, 7, 2, 2, 1, 1, -3, -3, 64, 8, 8, 1, 1, 0, 0, 64},
    {1, 5, 5, 64, 5, 5, 3, 3, 1, 1, 1, 1, -1, -1, 64, 5, 5, 1, 1, 0, 0, 64},
    // test_igemm_variants_prologue_epilogue
    {8, 16, 16, 64, 16, 16, 1, 1, 1, 1, 1, 1, 0, 0, 128, 16, 16, 1, 1, 0, 0, 128},
    {8, 16, 16, 64, 16, 16, 3, 3, 1, 1, 1, 1, -1, -1, 128, 16, 16, 1, 1, 0, 0, 128},
    {8, 16, 16, 64, 8, 8, 3, 3, 2, 2, 1, 1, -1, -1, 128, 8, 8, 1, 1, 0, 0, 128},
    // test_igemm_block_output_prologue
    {16, 16, 16, 256, 16, 16, 1, 1, 1, 1, 1, 1, 0, 0, 64, 16, 16, 1, 1, 0, 0, 64},
    {16, 8, 8, 512, 8, 8, 1, 1, 1, 1, 1, 1, 0, 0, 128, 8, 8, 1, 1, 0, 0, 128},
    {16, 4, 4, 1024, 4, 4, 1, 1, 1, 1, 1, 1, 0, 0, 256, 4, 4, 1, 1, 0, 0, 256},
    {16, 4, 4, 2048, 4, 4, 1, 1, 1, 1, 1, 1, 0, 0, 512, 4, 4, 1, 1, 0, 0, 512},
    // test_igemm_glds_variants
    {8, 16, 16, 64, 16, 16, 1, 1, 1, 1, 1, 1, 0, 0, 256, 16, 16, 1, 1, 0, 0, 256},
    {8, 16, 16, 64, 16, 16, 3, 3, 1, 1, 1, 1, -1, -1, 64, 16, 16, 1, 1, 0, 0, 64},
    {8, 16, 16, 128, 8, 8, 3, 3, 2, 2, 1, 1, -1, -1, 192, 8, 8, 1, 1, 0, 0, 192},
    {8, 16, 16, 128, 8, 8, 1, 1, 2, 2, 1, 1, 0, 0, 128, 8, 8, 1, 1, 0, 0, 128},
    {8, 16, 16, 128, 16, 16, 3, 3, 1, 1, 1, 1, -1, -1, 512, 16, 16, 1, 1, 0, 0, 512},
    {8, 32, 32, 64, 32, 32, 3, 3, 1, 1, 1, 1, -1, -1, 64, 32, 32, 1, 1, 0, 0, 64},
    {8, 32, 32, 128, 32, 32, 3, 3, 1, 1, 1, 1, -1, -1, 128, 32, 32, 1, 1, 0, 0, 128},
    // test_wgrad_glds_variants
    {8, 4, 4, 256, 4, 4, 3, 3, 1, 1, 1, 1, -1, -1, 512, 4, 4, 1, 1, 0, 0, 512},
    {8, 5, 5, 64, 5, 5, 3, 3, 1, 1, 1, 1, -1, -1, 64, 5, 5, 1, 1, 0, 0, 64},
    {8, 16, 16, 128, 16, 16, 3, 3, 1, 1, 1, 1, -1, -1, 128, 16, 16, 1, 1, 0, 0, 128},
    {8, 32, 32, 128, 32, 32, 3, 3, 1, 1, 1, 1, -1, -1, 64, 32, 32, 1, 1, 0, 0, 64},
    {8, 8, 8, 64, 8, 8, 3, 3, 1, 1, 1, 1, -1, -1, 128, 8, 8, 1, 1, 0, 0, 128},
    {8, 8, 8, 64, 4, 4, 3, 3, 2, 2, 1, 1, -1, -1, 64, 4, 4, 1, 1, 0, 0, 64},
    // stride-2 dgrad parity class (0, 0)
    {8, 8, 8, 128, 8, 8, 1, 1, 1, 1, -1, -1, 0, 0, 128, 16, 16, 2, 2, 0, 0, 128},
    // stride-2 dgrad parity class (0, 1)
    {8, 8, 8, 128, 8, 8, 1, 2, 1, 1, -1, -1, 0, 1, 128, 16, 16, 2, 2, 0, 1, 128},
    // stride-2 dgrad parity class (1, 0)
    {8, 8, 8, 128, 8, 8, 2, 1, 1, 1, -1, -1, 1, 0, 128, 16, 16, 2, 2, 1, 0, 128},
    // stride-2 dgrad parity class (1, 1)
    {8, 8, 8, 128, 8, 8, 2, 2, 1, 1, -1, -1, 1, 1, 128, 16, 16, 2, 2, 1, 1, 128},
    // stride-2 dgrad parity class (0, 0)
    {8, 16, 16, 128, 16, 16, 1, 1, 1, 1, -1, -1, 0, 0, 64, 32, 32, 2, 2, 0, 0, 64},
    // stride-2 dgrad parity class (0, 1)
    {8, 16, 16, 128, 16, 16, 1, 2, 1, 1, -1, -1, 0, 1, 64, 32, 32, 2, 2, 0, 1, 64},
    // stride-2 dgrad parity class (1, 0)
    {8, 16, 16, 128, 16, 16, 2, 1, 1, 1, -1, -1, 1, 0, 64, 32, 32, 2, 2, 1, 0, 64},
    // stride-2 dgrad parity class (1, 1)
    {8, 16, 16, 128, 16, 16, 2, 2, 1, 1, -1, -1, 1, 1, 64, 32, 32, 2, 2, 1, 1, 64},
    // stride-2 dgrad parity class (0, 0)
    {8, 8, 8, 256, 8, 8, 1, 1, 1, 1, -1, -1, 0, 0, 128, 16, 16, 2, 2, 0, 0, 128},
    {8, 4, 4, 256, 4, 4, 1, 1, 1, 1, -1, -1, 0, 0, 256, 8, 8, 2, 2, 0, 0, 256},
    // stride-2 dgrad parity class (0, 1)
    {8, 4, 4, 256, 4, 4, 1, 2, 1, 1, -1, -1, 0, 1, 256, 8, 8, 2, 2, 0, 1, 256},
    // stride-2 dgrad parity class (1, 0)
    {8, 4, 4, 256, 4, 4, 2, 1, 1, 1, -1, -1, 1, 0, 256, 8, 8, 2, 2, 1, 0, 256},
    // stride-2 dgrad parity class (1, 1)
    {8, 4, 4, 256, 4, 4, 2, 2, 1, 1, -1, -1, 1, 1, 256, 8, 8, 2, 2, 1, 1, 256},
    // test_wgrad_bn_backward_prologue_padded_channels (C = 8 stem)
    {16, 32, 32, 8, 32, 32, 3, 3, 1, 1, 1, 1, -1, -1, 64, 32, 32, 1, 1, 0, 0, 64},
    {16, 32, 32, 8, 36, 36, 3, 3, 1, 1, 1, 1, -3, -3, 64, 36, 36, 1, 1, 0, 0, 64},
    // rejected by LDS-DMA: C % 64 != 0
    {8, 16, 16, 96, 16, 16, 1, 1, 1, 1, 1, 1, 0, 0, 128, 16, 16, 1, 1, 0, 0, 128},
    {8, 16, 16, 32, 16, 16, 3, 3, 1, 1, 1, 1, -1, -1, 64, 16, 16, 1, 1, 0, 0, 64},
    // padded 3x3 off the patch geometry (C = 256): no prologue on LDS-DMA
    {8, 16, 16, 256, 16, 16, 3, 3, 1, 1, 1, 1, -1, -1, 256, 16, 16, 1, 1, 0, 0, 256},
    // patch kernel rejects OW = 8
    {8, 8, 8, 64, 8, 8, 3, 3, 1, 1, 1, 1, -1, -1, 64, 8, 8, 1, 1, 0, 0, 64},
    // patch kernel rejects OW = 64
    {4, 64, 64, 64, 64, 64, 3, 3, 1, 1, 1, 1, -1, -1, 64, 64, 64, 1, 1, 0, 0, 64},
};

template <class F>
unsigned mask_of(int n, F ok) {
  unsigned m = 0;
  for (int v = 0; v < n; ++v) m |= ok(v) ? 1u << v : 0u;
  return m;
}

void dump() {
  const int ni = igemm_num_variants(), nw = wgrad_num_variants();
  std::printf("[\n{\"igemm_variants\": %d, \"wgrad_variants\": %d}", ni, nw);
  for (int v = 0; v < ni; ++v)
    std::printf(",\n{\"igemm\": %d, \"bm\": %d, \"bn\": %d, \"glds\": %d, \"patch\": %d}", v,
                igemm_variant_bm(v), igemm_variant_bn(v), (int)igemm_variant_glds(v),
                (int)igemm_variant_patch(v));
  for (int v = 0; v < nw; ++v)
    std::printf(",\n{\"wgrad\": %d, \"glds\": %d, \"area\": %d}", v, (int)wgrad_variant_glds(v),
                wgrad_variant_area(v));
  for (const ConvGeom& g : DUMP_GEOMS) {
    std::printf(",\n{\"geom\": [");
    const int* p = &g.Nb;
    for (int i = 0; i < 22; ++i) std::printf("%s%d", i ? ", " : "", p[i]);
    std::printf("], \"igemm_ok\": [");  // (pro, bn_bwd_pro) = (0,0) (1,0) (0,1) (1,1)
    for (int c = 0; c < 4; ++c)
      std::printf("%s%u", c ? ", " : "",
                  mask_of(ni, [&](int v) { return igemm_variant_ok(v, g, c & 1, c >> 1); }));
    std::printf("], \"dual_ok\": %u, \"wgrad_ok\": [",
                mask_of(ni, [&](int v) { return igemm_dual_ok(v, g); }));
    for (int c = 0; c < 4; ++c)  // (pro, dy_pro) in the same order
      std::printf("%s%u", c ? ", " : "",
                  mask_of(nw, [&](int v) { return wgrad_variant_ok(v, g, c & 1, c >> 1); }));
    std::printf("], \"splits_tiles\": [");  // [variant, splits, tiles] of every admissible one
    const char* sep = "";
    for (int v = 0; v < nw; ++v)
      if (wgrad_variant_ok(v, g, false, false)) {
        std::printf("%s[%d, %d, %d]", sep, v, wgrad_splits(g, v), wgrad_tiles(g, v));
        sep = ", ";
      }
    std::printf("]}");
  }
  std::printf("\n]\n");
}

#ifndef HOST_CHECK_V1_API
// the epilogue argument of igemm_variant_ok: modes 0-3 change nothing, and the BN-backward
// prologue with the mode-4 epilogue leaves the LDS-DMA tiles of at most 256 x 128
void check_epilogue_rule() {
  for (const ConvGeom& g : DUMP_GEOMS)
    for (int v = 0; v < igemm_num_variants(); ++v) {
      const bool big = igemm_variant_glds(v) &&
                       igemm_variant_bm(v) * igemm_variant_bn(v) > 256 * 128;
      for (int c = 0; c < 4; ++c) {
        const bool pro = c & 1, bnb = c >> 1, base = igemm_variant_ok(v, g, pro, bnb);
        for (int e = 0; e < 4; ++e)
          EXPECT(igemm_variant_ok(v, g, pro, bnb, e) == base, "variant %d epilogue %d", v, e);
        if (bnb)
          EXPECT(igemm_variant_ok(v, g, pro, true, 4) == (base && !big), "variant %d mode 4", v);
      }
    }
}
#endif

}  // namespace

int main(int argc, char** argv) {
  if (argc > 1 && !std::strcmp(argv[1], "--dump")) {
    unsetenv("SIMCLR_WGRAD_TARGET_PCT");  // the recorded split counts are the default target's
    dump();
    return 0;
  }
#ifndef HOST_CHECK_V1_API
  check_epilogue_rule();
#endif
  for (int batch : {64, 1024}) {
    check_net("resnet50-cifar", true, 32, false, batch);
    check_net("resnet18-cifar", false, 36, false, batch);
    check_net("resnet50-imagenet@32", true, 32, true, batch);
  }
  check_net("resnet50-imagenet@224", true, 224, true, 256);
  for (int R : {128, 1024, 8192})
    for (int Cc : {R, 8 * R}) {
      EXPECT(ntxent_fwd_splits(R, Cc) >= 1, "nt fwd splits");
      EXPECT(ntxent_bwd_splits(R, Cc) >= 1, "nt bwd splits");
    }
  for (int N : {10, 5000, 50000}) EXPECT(class_sums_groups(N) >= 1, "class sums groups");
  EXPECT(class_sums_lds(100) <= 64 * 1024, "class sums lds");
  EXPECT(colsum_groups(1024) >= 1 && colsum_groups(1) >= 1, "colsum groups");
  std::printf("host_check: %d failure(s)\n", failures);
  return failures ? 1 : 0;
}
