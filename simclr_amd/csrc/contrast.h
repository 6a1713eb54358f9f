// The online log-sum-exp of the contrastive forward kernels (ntxent.hip, nnclr.hip) and their
// dispatch on the embedding width.  A row's softmax denominator is carried as (m, l) =
// (running max, Σ exp(s − m)); the three functions below are the only places that update one,
// so the kernels' partials ([split][row][m, l, ...]) agree bit for bit wherever they share a
// merge order: lanes by lse_merge_lanes over off = 16, 32, then splits by lse_merge_split in
// ascending order.
#pragma once
#include "common.h"

// one more logit
__device__ __forceinline__ void lse_push(float& m, float& l, float v) {
  if (v > m) {
    l = l * __expf(m - v) + 1.f;
    m = v;
  } else {
    l += __expf(v - m);
  }
}

// (m, l) of the lane `off` away merged into this lane's: the 4 lane groups holding one row
__device__ __forceinline__ void lse_merge_lanes(float& m, float& l, int off) {
  const float m2 = __shfl_xor(m, off, 64);
  const float l2 = __shfl_xor(l, off, 64);
  const float mn = fmaxf(m, m2);
  l = (mn == -INFINITY) ? 0.f : l * __expf(m - mn) + l2 * __expf(m2 - mn);
  m = mn;
}

// a split's partial p = (m2, l2, ...) merged into (m, l)
__device__ __forceinline__ void lse_merge_split(float& m, float& l, const float* p) {
  const float mn = fmaxf(m, p[0]);
  if (mn != -INFINITY) l = l * __expf(m - mn) + p[1] * __expf(p[0] - mn);
  m = mn;
}

// Runs the statement(s) after `what` with DD = D as a constant expression; D is one of the
// widths the kernels are instantiated for.
#define DISPATCH_D(D, what, ...)                                         \
  switch (D) {                                                           \
    case 32: { constexpr int DD = 32; __VA_ARGS__; } break;              \
    case 64: { constexpr int DD = 64; __VA_ARGS__; } break;              \
    case 128: { constexpr int DD = 128; __VA_ARGS__; } break;            \
    case 256: { constexpr int DD = 256; __VA_ARGS__; } break;            \
    default: fprintf(stderr, what ": unsupported D=%d\n", D); abort();   \
  }
