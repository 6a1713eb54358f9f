// Shared device helpers for the gfx950 (MI355X / CDNA4) kernels of simclr_amd.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef short i16x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

#define LDS_PTR(T, p) ((__attribute__((address_space(3))) T*)(p))

__device__ __forceinline__ float bf2f(uint16_t b) { return __uint_as_float(((uint32_t)b) << 16); }

// Round-to-nearest-even, NaN-preserving (lowers to v_cvt_pk_bf16_f32 on gfx950).
__device__ __forceinline__ uint16_t f2bf(float f) {
  __bf16 h = (__bf16)f;
  return __builtin_bit_cast(uint16_t, h);
}

__device__ __forceinline__ uint32_t pack2bf(float lo, float hi) {
  return (uint32_t)f2bf(lo) | ((uint32_t)f2bf(hi) << 16);
}

__device__ __forceinline__ float lo_bf(uint32_t w) { return __uint_as_float(w << 16); }
__device__ __forceinline__ float hi_bf(uint32_t w) { return __uint_as_float(w & 0xffff0000u); }

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// Transposed staging of a [32 rows][64 columns] bf16 tile into LDS as Xs[column][row] (row stride
// XT_LD), the K-contiguous B operand of an MFMA whose K runs over the rows.  Thread tid of 256 owns
// the 16-byte chunk tid & 7 of tile row tid >> 3: xt_load reads it for the tile that starts at row
// k0 (row(k): the tile's first column in row k; zeros for the rows from kend on, for which row is
// not called), xt_store scatters its eight values.
constexpr int XT_ROWS = 32, XT_LD = XT_ROWS + 8;

template <class RowPtr>
__device__ __forceinline__ u32x4 xt_load(int k0, int kend, int tid, RowPtr row) {
  const int k = k0 + (tid >> 3);
  if (k >= kend) return (u32x4){0u, 0u, 0u, 0u};
  return *(const u32x4*)(row(k) + (tid & 7) * 8);
}

__device__ __forceinline__ void xt_store(uint16_t* Xs, int tid, u32x4 rx) {
  const int sk = tid >> 3, sc = tid & 7;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    Xs[(sc * 8 + 2 * i) * XT_LD + sk] = (uint16_t)(rx[i] & 0xffffu);
    Xs[(sc * 8 + 2 * i + 1) * XT_LD + sk] = (uint16_t)(rx[i] >> 16);
  }
}

// Bijective XCD-aware remap of a linear workgroup id (cdna_hip_programming.md §5 / T1):
// consecutive *logical* ids land on the same XCD (blocks b and b+8 share an XCD).
__device__ __forceinline__ int xcd_remap(int bid, int nwg) {
  const int q = nwg / 8, r = nwg % 8;
  const int xcd = bid % 8;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + bid / 8;
}

#define HIP_CHECK_LAUNCH()                                                        \
  do {                                                                            \
    hipError_t e__ = hipGetLastError();                                           \
    if (e__ != hipSuccess) {                                                      \
      fprintf(stderr, "HIP launch error %s at %s:%d\n", hipGetErrorString(e__),   \
              __FILE__, __LINE__);                                                \
      abort();                                                                    \
    }                                                                             \
  } while (0)
