// On-device SimCLR augmentation (gfx950): one workgroup per (image, view).
//
// Reference: create_simclr_data_augmentation (/root/reference/dataset.py:19-38) run by 8 CPU
// DataLoader workers per GPU through PIL:
//   RandomResizedCrop(32, scale=(0.08,1), ratio=(3/4,4/3), bilinear) → RandomHorizontalFlip(0.5)
//   → RandomApply([ColorJitter(0.8s,0.8s,0.8s,0.2s)], p=0.8) → RandomGrayscale(0.2) → ToTensor.
// The uint8 dataset lives in HBM once (CIFAR-10 = 150 MB); per step only an index vector moves.
// Parameters follow torchvision's samplers (10-attempt rejection sampling with the central-crop
// fallback, jitter factors U[max(0,1-x), 1+x], random op order per image); pixel math follows
// PIL (half-pixel-centre bilinear with edge clamp, uint8 rounding between ops, blend truncation,
// ITU-R 601-2 luma with PIL's fixed-point rounding, contrast against the rounded mean luma).
// Hue uses a float HSV round trip (PIL's uint8 HSV differs by quantisation only).
// Output: bf16 NHWC with the channel dim zero-padded to Cpad (8) for 16-byte conv gathers.
// RNG: counter-based splitmix64 keyed by (seed, step counter, view, dataset index) — independent
// of rank count and launch order.
#include <math.h>
#include "common.h"
#include "kernels.h"

namespace {

__device__ __forceinline__ uint64_t splitmix64(uint64_t x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

struct Rng {
  uint64_t key;
  uint64_t ctr;
  __device__ float uniform() {  // [0, 1)
    const uint64_t r = splitmix64(key ^ (0xD1B54A32D192ED03ull * (++ctr)));
    return (float)(r >> 40) * (1.0f / 16777216.0f);
  }
  __device__ float uniform(float a, float b) { return a + (b - a) * uniform(); }
  __device__ int randint(int lo, int hi_excl) {  // [lo, hi)
    const uint64_t r = splitmix64(key ^ (0xD1B54A32D192ED03ull * (++ctr)));
    return lo + (int)(r % (uint64_t)(hi_excl - lo));
  }
};

struct AugParams {
  int ci, cj, ch, cw;   // crop
  int flip;
  int jitter;           // jitter applied
  int order[4];         // 0 brightness 1 contrast 2 saturation 3 hue
  float fb, fc, fs, fh;
  int gray;
};

__device__ void sample_params(Rng& rng, int H, int W, float strength, AugParams& P) {
  // RandomResizedCrop.get_params
  const float area = (float)(H * W);
  const float lr0 = logf(3.f / 4.f), lr1 = logf(4.f / 3.f);
  bool found = false;
  for (int t = 0; t < 10 && !found; ++t) {
    const float target = area * rng.uniform(0.08f, 1.0f);
    const float ar = expf(rng.uniform(lr0, lr1));
    const int w = (int)rintf(sqrtf(target * ar));
    const int h = (int)rintf(sqrtf(target / ar));
    if (w > 0 && w <= W && h > 0 && h <= H) {
      P.ci = rng.randint(0, H - h + 1);
      P.cj = rng.randint(0, W - w + 1);
      P.ch = h;
      P.cw = w;
      found = true;
    }
  }
  if (!found) {
    const float in_ratio = (float)W / (float)H;
    int w, h;
    if (in_ratio < 3.f / 4.f) {
      w = W; h = (int)rintf(w / (3.f / 4.f));
    } else if (in_ratio > 4.f / 3.f) {
      h = H; w = (int)rintf(h * (4.f / 3.f));
    } else {
      w = W; h = H;
    }
    P.ci = (H - h) / 2; P.cj = (W - w) / 2; P.ch = h; P.cw = w;
  }
  P.flip = rng.uniform() < 0.5f;
  // RandomApply(p=0.8): applied unless p < rand
  P.jitter = !(0.8f < rng.uniform());
  // ColorJitter.get_params: randperm(4) then factors
  int ord[4] = {0, 1, 2, 3};
  for (int i = 3; i > 0; --i) {
    const int j = rng.randint(0, i + 1);
    const int t = ord[i]; ord[i] = ord[j]; ord[j] = t;
  }
  for (int i = 0; i < 4; ++i) P.order[i] = ord[i];
  const float b = 0.8f * strength, c = 0.8f * strength, s = 0.8f * strength, h = 0.2f * strength;
  P.fb = rng.uniform(fmaxf(0.f, 1.f - b), 1.f + b);
  P.fc = rng.uniform(fmaxf(0.f, 1.f - c), 1.f + c);
  P.fs = rng.uniform(fmaxf(0.f, 1.f - s), 1.f + s);
  P.fh = rng.uniform(-h, h);
  P.gray = rng.uniform() < 0.2f;
}

__device__ __forceinline__ float clip_trunc(float v) {  // PIL blend: clip then truncate to uint8
  return v <= 0.f ? 0.f : (v >= 255.f ? 255.f : floorf(v));
}

__device__ __forceinline__ int luma(float r, float g, float b) {  // PIL L24 fixed point
  return ((int)r * 19595 + (int)g * 38470 + (int)b * 7471 + 0x8000) >> 16;
}

__device__ void rgb2hsv(float r, float g, float b, float& h, float& s, float& v) {
  const float mx = fmaxf(r, fmaxf(g, b)), mn = fminf(r, fminf(g, b));
  v = mx;
  const float d = mx - mn;
  s = mx > 0.f ? d / mx : 0.f;
  if (d <= 0.f) { h = 0.f; return; }
  float hh;
  if (mx == r) hh = (g - b) / d;
  else if (mx == g) hh = 2.f + (b - r) / d;
  else hh = 4.f + (r - g) / d;
  hh /= 6.f;
  h = hh - floorf(hh);
}

__device__ void hsv2rgb(float h, float s, float v, float& r, float& g, float& b) {
  const float h6 = h * 6.f;
  const int i = ((int)floorf(h6)) % 6;
  const float f = h6 - floorf(h6);
  const float p = v * (1.f - s), q = v * (1.f - s * f), t = v * (1.f - s * (1.f - f));
  switch (i) {
    case 0: r = v; g = t; b = p; break;
    case 1: r = q; g = v; b = p; break;
    case 2: r = p; g = v; b = t; break;
    case 3: r = p; g = q; b = v; break;
    case 4: r = t; g = p; b = v; break;
    default: r = v; g = p; b = q; break;
  }
}

constexpr int AUG_THREADS = 256;
constexpr int MAX_PIX_PER_THREAD = 16;  // up to 64x64 outputs

// ---- Gaussian blur (SimCLR's recipe for larger images; opt-in, blur_kernel != 0) ------------
// RandomApply([GaussianBlur(ks, sigma ~ U[0.1, 2.0])], p = 0.5) after grayscale, on the integer
// 0..255 image, as torchvision's gaussian_blur of a uint8 image: taps exp(-0.5 (x / sigma)^2)
// over their fp32 sum, a horizontal then a vertical pass (taps accumulated in index order, the
// intermediate kept in fp32), reflect padding without edge repeat, clip(floor(v + 0.5), 0, 255).
// The two draws (applied, sigma) follow the grayscale draw and are made only by the BLUR
// instantiations, so every other parameter of an image is the same with blur on or off; the
// BLUR = false instantiations are the kernels as they were (no blur state, no dynamic LDS).
// Blur reads neighbouring pixels, so a blurred image is staged in dynamic LDS, which starts with
// this header (written by thread 0 with the parameters).
constexpr int AUG_MAX_BLUR_KS = 33;
constexpr int BLUR_HDR_BYTES = 256;
constexpr int BLUR_LDS_BYTES = 60 * 1024;  // dynamic LDS of a blur launch (64 KB with the static)
struct BlurHdr {
  int blur;  // applied to this image
  float sigma;
  float w[AUG_MAX_BLUR_KS];
};
static_assert(sizeof(BlurHdr) <= BLUR_HDR_BYTES, "blur header");

__device__ __forceinline__ char* blur_lds() {
  extern __shared__ __attribute__((aligned(16))) char aug_lds[];
  return aug_lds;
}

__device__ void sample_blur(Rng& rng, int ks, BlurHdr& h) {
  h.blur = !(0.5f < rng.uniform());  // RandomApply(p=0.5)
  // a + (b - a) u rounded after the product and after the sum (no fused multiply-add), so that
  // params_out's sigma is the NumPy twin's bit for bit
  {
#pragma clang fp contract(off)
    const float scaled = (2.0f - 0.1f) * rng.uniform();
    h.sigma = 0.1f + scaled;
  }
  const int r = ks >> 1;
  float s = 0.f;
  for (int i = 0; i < ks; ++i) {
    const float q = (float)(i - r) / h.sigma;
    const float e = expf(-0.5f * q * q);
    h.w[i] = e;
    s += e;
  }
  for (int i = 0; i < ks; ++i) h.w[i] /= s;
}

__device__ __forceinline__ int reflect(int i, int n) {  // -1 -> 1, n -> n - 2
  i = i < 0 ? -i : i;
  return i >= n ? 2 * (n - 1) - i : i;
}

__device__ __forceinline__ float round_u8(float v) {
  return fminf(fmaxf(floorf(v + 0.5f), 0.f), 255.f);
}

// Blur one register-resident plane of k_augment through two fp32 LDS planes [OH*OW].  Reached by
// every thread of the block (the blur decision is per image); the caller's next call may write
// `pa` at once: all threads are past the horizontal pass, the only reader of `pa`.
__device__ __forceinline__ void blur_plane(float (&X)[MAX_PIX_PER_THREAD], int myn, int OH, int OW,
                                           int ks, const float* w, float* pa, float* pb) {
  const int r = ks >> 1;
#pragma unroll
  for (int k = 0; k < MAX_PIX_PER_THREAD; ++k) {
    if (k >= myn) break;
    pa[threadIdx.x + k * AUG_THREADS] = X[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < MAX_PIX_PER_THREAD; ++k) {
    if (k >= myn) break;
    const int p = threadIdx.x + k * AUG_THREADS;
    const int oy = p / OW, ox = p - oy * OW;
    const float* row = pa + oy * OW;
    float acc = 0.f;
    for (int t = 0; t < ks; ++t) acc += w[t] * row[reflect(ox + t - r, OW)];
    pb[p] = acc;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < MAX_PIX_PER_THREAD; ++k) {
    if (k >= myn) break;
    const int p = threadIdx.x + k * AUG_THREADS;
    const int oy = p / OW, ox = p - oy * OW;
    float acc = 0.f;
    for (int t = 0; t < ks; ++t) acc += w[t] * pb[reflect(oy + t - r, OH) * OW + ox];
    X[k] = round_u8(acc);
  }
}

template <bool BLUR>
__global__ __launch_bounds__(AUG_THREADS) void k_augment(const uint8_t* __restrict__ images,
                                                         const int64_t* __restrict__ indices,
                                                         int n, int H, int W, int OH, int OW,
                                                         int Cpad, float strength, uint64_t seed,
                                                         uint64_t counter, int view_offset,
                                                         int flags, uint16_t* __restrict__ out,
                                                         float* __restrict__ params_out,
                                                         int blur_ks) {
  __shared__ AugParams P;
  __shared__ int red[AUG_THREADS / 64];
  const int b = blockIdx.x, view = blockIdx.y + view_offset;
  const int64_t idx = indices ? indices[b] : (int64_t)b;
  const uint8_t* img = images + (size_t)idx * H * W * 3;
  const bool augment = flags & 1;
  if (threadIdx.x == 0) {
    float sigma_out = 0.f;
    if (augment) {
      Rng rng{splitmix64(seed ^ splitmix64(counter * 0x9E3779B97F4A7C15ull + (uint64_t)view) ^
                         splitmix64((uint64_t)idx + 0x632BE59BD9B4E019ull)), 0};
      sample_params(rng, H, W, strength, P);
      if constexpr (BLUR) {
        BlurHdr& bh = *(BlurHdr*)blur_lds();
        sample_blur(rng, blur_ks, bh);
        sigma_out = bh.blur ? bh.sigma : 0.f;
      }
    } else {
      P.ci = 0; P.cj = 0; P.ch = H; P.cw = W; P.flip = 0; P.jitter = 0; P.gray = 0;
      P.fb = P.fc = P.fs = 1.f; P.fh = 0.f;
      for (int i = 0; i < 4; ++i) P.order[i] = i;
      if constexpr (BLUR) ((BlurHdr*)blur_lds())->blur = 0;
    }
    if (params_out) {
      float* po = params_out + ((size_t)blockIdx.y * n + b) * 16;
      po[0] = P.ci; po[1] = P.cj; po[2] = P.ch; po[3] = P.cw; po[4] = P.flip; po[5] = P.jitter;
      for (int i = 0; i < 4; ++i) po[6 + i] = P.order[i];
      po[10] = P.fb; po[11] = P.fc; po[12] = P.fs; po[13] = P.fh; po[14] = P.gray;
      po[15] = sigma_out;
    }
  }
  __syncthreads();
  const int npix = OH * OW;
  float R[MAX_PIX_PER_THREAD], G[MAX_PIX_PER_THREAD], B[MAX_PIX_PER_THREAD];
  const int myn = (npix - (int)threadIdx.x + AUG_THREADS - 1) / AUG_THREADS;
  // resized crop (+ flip), rounded to uint8 like PIL
  const float sy = (float)P.ch / OH, sx = (float)P.cw / OW;
#pragma unroll
  for (int k = 0; k < MAX_PIX_PER_THREAD; ++k) {
    if (k >= myn) break;
    const int p = threadIdx.x + k * AUG_THREADS;
    const int oy = p / OW;
    int ox = p - oy * OW;
    if (P.flip) ox = OW - 1 - ox;
    float fy = (oy + 0.5f) * sy - 0.5f;
    float fx = (ox + 0.5f) * sx - 0.5f;
    fy = fminf(fmaxf(fy, 0.f), (float)(P.ch - 1));
    fx = fminf(fmaxf(fx, 0.f), (float)(P.cw - 1));
    const int y0 = (int)floorf(fy), x0 = (int)floorf(fx);
    const int y1 = min(y0 + 1, P.ch - 1), x1 = min(x0 + 1, P.cw - 1);
    const float wy = fy - y0, wx = fx - x0;
    const uint8_t* p00 = img + ((size_t)(P.ci + y0) * W + (P.cj + x0)) * 3;
    const uint8_t* p01 = img + ((size_t)(P.ci + y0) * W + (P.cj + x1)) * 3;
    const uint8_t* p10 = img + ((size_t)(P.ci + y1) * W + (P.cj + x0)) * 3;
    const uint8_t* p11 = img + ((size_t)(P.ci + y1) * W + (P.cj + x1)) * 3;
    float c3[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float top = p00[c] + wx * (p01[c] - p00[c]);
      const float bot = p10[c] + wx * (p11[c] - p10[c]);
      const float v = top + wy * (bot - top);
      c3[c] = fminf(fmaxf(floorf(v + 0.5f), 0.f), 255.f);
    }
    R[k] = c3[0]; G[k] = c3[1]; B[k] = c3[2];
  }
  if (P.jitter) {
    for (int oi = 0; oi < 4; ++oi) {
      const int op = P.order[oi];
      if (op == 0) {  // brightness: blend(black, img, f)
#pragma unroll
        for (int k = 0; k < MAX_PIX_PER_THREAD; ++k) {
          if (k >= myn) break;
          R[k] = clip_trunc(R[k] * P.fb); G[k] = clip_trunc(G[k] * P.fb); B[k] = clip_trunc(B[k] * P.fb);
        }
      } else if (op == 1) {  // contrast: blend(mean luma, img, f)
        int s = 0;
#pragma unroll
        for (int k = 0; k < MAX_PIX_PER_THREAD; ++k) {
          if (k >= myn) break;
          s += luma(R[k], G[k], B[k]);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
        __syncthreads();
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
        __syncthreads();
        int tot = 0;
        for (int w = 0; w < AUG_THREADS / 64; ++w) tot += red[w];
        const float mean = floorf((float)tot / npix + 0.5f);
#pragma unroll
        for (int k = 0; k < MAX_PIX_PER_THREAD; ++k) {
          if (k >= myn) break;
          R[k] = clip_trunc(mean + P.fc * (R[k] - mean));
          G[k] = clip_trunc(mean + P.fc * (G[k] - mean));
          B[k] = clip_trunc(mean + P.fc * (B[k] - mean));
        }
      } else if (op == 2) {  // saturation: blend(gray, img, f)
#pragma unroll
        for (int k = 0; k < MAX_PIX_PER_THREAD; ++k) {
          if (k >= myn) break;
          const float l = (float)luma(R[k], G[k], B[k]);
          R[k] = clip_trunc(l + P.fs * (R[k] - l));
          G[k] = clip_trunc(l + P.fs * (G[k] - l));
          B[k] = clip_trunc(l + P.fs * (B[k] - l));
        }
      } else {  // hue
#pragma unroll
        for (int k = 0; k < MAX_PIX_PER_THREAD; ++k) {
          if (k >= myn) break;
          float h, s, v, r, g, bb;
          rgb2hsv(R[k] / 255.f, G[k] / 255.f, B[k] / 255.f, h, s, v);
          h += P.fh;
          h -= floorf(h);
          hsv2rgb(h, s, v, r, g, bb);
          R[k] = fminf(fmaxf(floorf(r * 255.f + 0.5f), 0.f), 255.f);
          G[k] = fminf(fmaxf(floorf(g * 255.f + 0.5f), 0.f), 255.f);
          B[k] = fminf(fmaxf(floorf(bb * 255.f + 0.5f), 0.f), 255.f);
        }
      }
    }
  }
  if constexpr (BLUR) {
    const BlurHdr& bh = *(const BlurHdr*)blur_lds();
    if (bh.blur) {  // per image: every thread of the block takes this branch or none does
      float* pa = (float*)(blur_lds() + BLUR_HDR_BYTES);
      float* pb = pa + npix;
      if (P.gray) {  // grayscale comes before the blur; R = G = B, so one plane is filtered
#pragma unroll
        for (int k = 0; k < MAX_PIX_PER_THREAD; ++k) {
          if (k >= myn) break;
          R[k] = (float)luma(R[k], G[k], B[k]);
        }
      }
      blur_plane(R, myn, OH, OW, blur_ks, bh.w, pa, pb);
      if (P.gray) {  // (the store below takes the luma of (l, l, l), which is l)
#pragma unroll
        for (int k = 0; k < MAX_PIX_PER_THREAD; ++k) {
          if (k >= myn) break;
          G[k] = B[k] = R[k];
        }
      } else {
        blur_plane(G, myn, OH, OW, blur_ks, bh.w, pa, pb);
        blur_plane(B, myn, OH, OW, blur_ks, bh.w, pa, pb);
      }
    }
  }
  const size_t obase = ((size_t)blockIdx.y * n + b) * npix;
  const float inv255 = 1.f / 255.f;
#pragma unroll
  for (int k = 0; k < MAX_PIX_PER_THREAD; ++k) {
    if (k >= myn) break;
    const int p = threadIdx.x + k * AUG_THREADS;
    float r = R[k], g = G[k], bb = B[k];
    if (P.gray) {
      const float l = (float)luma(r, g, bb);
      r = g = bb = l;
    }
    uint16_t* o = out + (obase + p) * Cpad;
    if (Cpad == 8) {
      u32x4 w;
      w[0] = pack2bf(r * inv255, g * inv255);
      w[1] = pack2bf(bb * inv255, 0.f);
      w[2] = 0; w[3] = 0;
      *(u32x4*)o = w;
    } else {
      o[0] = f2bf(r * inv255); o[1] = f2bf(g * inv255); o[2] = f2bf(bb * inv255);
      for (int c = 3; c < Cpad; ++c) o[c] = 0;
    }
  }
}

// ---- ImageNet-shape outputs (BASELINE config 5: 224x224) --------------------------------
// The register-resident kernel above holds every output pixel of an image (<= 64x64) across
// the colour ops, because contrast blends against the mean luma of the image as it is at that
// point of the random op order.  For large outputs the block instead walks the pixels twice:
// pass 1 recomputes crop + the ops before contrast and reduces the luma sum; pass 2 recomputes
// them, applies contrast with the mean and the remaining ops and writes.  Every per-pixel op is
// deterministic, so both passes see identical values (recompute instead of a scratch image).
__device__ __forceinline__ void crop_pixel(const AugParams& P, const uint8_t* img, int W, int OH,
                                           int OW, int p, float& r, float& g, float& b) {
  const float sy = (float)P.ch / OH, sx = (float)P.cw / OW;
  const int oy = p / OW;
  int ox = p - oy * OW;
  if (P.flip) ox = OW - 1 - ox;
  float fy = (oy + 0.5f) * sy - 0.5f;
  float fx = (ox + 0.5f) * sx - 0.5f;
  fy = fminf(fmaxf(fy, 0.f), (float)(P.ch - 1));
  fx = fminf(fmaxf(fx, 0.f), (float)(P.cw - 1));
  const int y0 = (int)floorf(fy), x0 = (int)floorf(fx);
  const int y1 = min(y0 + 1, P.ch - 1), x1 = min(x0 + 1, P.cw - 1);
  const float wy = fy - y0, wx = fx - x0;
  const uint8_t* p00 = img + ((size_t)(P.ci + y0) * W + (P.cj + x0)) * 3;
  const uint8_t* p01 = img + ((size_t)(P.ci + y0) * W + (P.cj + x1)) * 3;
  const uint8_t* p10 = img + ((size_t)(P.ci + y1) * W + (P.cj + x0)) * 3;
  const uint8_t* p11 = img + ((size_t)(P.ci + y1) * W + (P.cj + x1)) * 3;
  float c3[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float top = p00[c] + wx * (p01[c] - p00[c]);
    const float bot = p10[c] + wx * (p11[c] - p10[c]);
    const float v = top + wy * (bot - top);
    c3[c] = fminf(fmaxf(floorf(v + 0.5f), 0.f), 255.f);
  }
  r = c3[0]; g = c3[1]; b = c3[2];
}

// one colour op (brightness / saturation / hue) on one pixel; contrast is handled by the caller
__device__ __forceinline__ void pixel_op(const AugParams& P, int op, float& R, float& G,
                                         float& B) {
  if (op == 0) {
    R = clip_trunc(R * P.fb); G = clip_trunc(G * P.fb); B = clip_trunc(B * P.fb);
  } else if (op == 2) {
    const float l = (float)luma(R, G, B);
    R = clip_trunc(l + P.fs * (R - l));
    G = clip_trunc(l + P.fs * (G - l));
    B = clip_trunc(l + P.fs * (B - l));
  } else if (op == 3) {
    float h, s, v, r, g, bb;
    rgb2hsv(R / 255.f, G / 255.f, B / 255.f, h, s, v);
    h += P.fh;
    h -= floorf(h);
    hsv2rgb(h, s, v, r, g, bb);
    R = fminf(fmaxf(floorf(r * 255.f + 0.5f), 0.f), 255.f);
    G = fminf(fmaxf(floorf(g * 255.f + 0.5f), 0.f), 255.f);
    B = fminf(fmaxf(floorf(bb * 255.f + 0.5f), 0.f), 255.f);
  }
}

// A pass-2 pixel: crop, the colour ops with contrast at position kc against `mean`, grayscale.
__device__ __forceinline__ void final_pixel(const AugParams& P, const uint8_t* img, int W, int OH,
                                            int OW, int p, int kc, float mean, float& r, float& g,
                                            float& bb) {
  crop_pixel(P, img, W, OH, OW, p, r, g, bb);
  if (P.jitter)
    for (int i = 0; i < 4; ++i) {
      if (i == kc) {
        r = clip_trunc(mean + P.fc * (r - mean));
        g = clip_trunc(mean + P.fc * (g - mean));
        bb = clip_trunc(mean + P.fc * (bb - mean));
      } else {
        pixel_op(P, P.order[i], r, g, bb);
      }
    }
  if (P.gray) {
    const float l = (float)luma(r, g, bb);
    r = g = bb = l;
  }
}

__device__ __forceinline__ void store_pixel(uint16_t* o, int Cpad, float r, float g, float bb) {
  const float inv255 = 1.f / 255.f;
  if (Cpad == 8) {
    u32x4 w;
    w[0] = pack2bf(r * inv255, g * inv255);
    w[1] = pack2bf(bb * inv255, 0.f);
    w[2] = 0; w[3] = 0;
    *(u32x4*)o = w;
  } else {
    o[0] = f2bf(r * inv255); o[1] = f2bf(g * inv255); o[2] = f2bf(bb * inv255);
    for (int c = 3; c < Cpad; ++c) o[c] = 0;
  }
}

// Blurred image of k_augment_large.  224x224x3 with an fp32 intermediate does not fit in LDS, so
// the block walks bands of `band` output rows.  Per band it recomputes the post-colour pixels of
// the band's rows and of the (ks-1)/2 halo rows above and below that lie inside the image (rows
// outside are reflections of staged rows, taken by index in the vertical pass) into three uint8
// planes (the values are integers 0..255), then per channel filters all staged rows horizontally
// into one fp32 plane and the band's rows vertically out of it, back into the channel's uint8
// plane, which the horizontal pass of that channel has finished reading; a gray image filters
// one plane.  LDS: header + rows * OW * (3 + 4) bytes with rows = band + ks - 1, within
// BLUR_LDS_BYTES: at OW 224 / ks 23 that is 39 rows, band 17, so the colour pipeline runs over
// (band + ks - 1) / band = 2.3 times the pixels of an unblurred image (augment_blur_band).
__device__ __forceinline__ void blur_bands(const AugParams& P, const BlurHdr& bh,
                                           const uint8_t* img, int W, int OH, int OW, int Cpad,
                                           int kc, float mean, int ks, int band, int rows,
                                           uint16_t* out, size_t obase) {
  float* f = (float*)(blur_lds() + BLUR_HDR_BYTES);   // [rows][OW] horizontally filtered
  uint8_t* u = (uint8_t*)(f + (size_t)rows * OW);     // [3][rows][OW] staged, then blurred
  const int plane = rows * OW;
  const int r = ks >> 1;
  const int nch = P.gray ? 1 : 3;
  for (int y0 = 0; y0 < OH; y0 += band) {
    const int nb = min(band, OH - y0);
    const int lo = max(0, y0 - r), hi = min(OH - 1, y0 + nb - 1 + r);
    const int nst = (hi - lo + 1) * OW;  // staged pixels, <= rows * OW
    __syncthreads();                     // the previous band's stores have read the planes
    for (int q = threadIdx.x; q < nst; q += AUG_THREADS) {
      float cr, cg, cb;
      final_pixel(P, img, W, OH, OW, lo * OW + q, kc, mean, cr, cg, cb);
      u[q] = (uint8_t)cr; u[plane + q] = (uint8_t)cg; u[2 * plane + q] = (uint8_t)cb;
    }
    __syncthreads();
    for (int c = 0; c < nch; ++c) {
      uint8_t* uc = u + c * plane;
      for (int q = threadIdx.x; q < nst; q += AUG_THREADS) {
        const int j = q / OW, x = q - j * OW;
        const uint8_t* row = uc + j * OW;
        float acc = 0.f;
        for (int t = 0; t < ks; ++t) acc += bh.w[t] * (float)row[reflect(x + t - r, OW)];
        f[q] = acc;
      }
      __syncthreads();
      for (int q = threadIdx.x; q < nb * OW; q += AUG_THREADS) {
        const int j = q / OW, x = q - j * OW;
        const int y = y0 + j;
        float acc = 0.f;
        for (int t = 0; t < ks; ++t) acc += bh.w[t] * f[(reflect(y + t - r, OH) - lo) * OW + x];
        uc[(y - lo) * OW + x] = (uint8_t)round_u8(acc);
      }
      __syncthreads();
    }
    for (int q = threadIdx.x; q < nb * OW; q += AUG_THREADS) {
      const int s = (y0 - lo) * OW + q;
      const float cr = (float)u[s];
      const float cg = P.gray ? cr : (float)u[plane + s];
      const float cb = P.gray ? cr : (float)u[2 * plane + s];
      store_pixel(out + (obase + (size_t)y0 * OW + q) * Cpad, Cpad, cr, cg, cb);
    }
  }
}

template <bool BLUR>
__global__ __launch_bounds__(AUG_THREADS) void k_augment_large(
    const uint8_t* __restrict__ images, const int64_t* __restrict__ indices, int n, int H, int W,
    int OH, int OW, int Cpad, float strength, uint64_t seed, uint64_t counter, int view_offset,
    int flags, uint16_t* __restrict__ out, float* __restrict__ params_out, int blur_ks,
    int blur_band, int blur_rows) {
  __shared__ AugParams P;
  __shared__ long long red[AUG_THREADS / 64];
  const int b = blockIdx.x, view = blockIdx.y + view_offset;
  const int64_t idx = indices ? indices[b] : (int64_t)b;
  const uint8_t* img = images + (size_t)idx * H * W * 3;
  if (threadIdx.x == 0) {
    float sigma_out = 0.f;
    if (flags & 1) {
      Rng rng{splitmix64(seed ^ splitmix64(counter * 0x9E3779B97F4A7C15ull + (uint64_t)view) ^
                         splitmix64((uint64_t)idx + 0x632BE59BD9B4E019ull)), 0};
      sample_params(rng, H, W, strength, P);
      if constexpr (BLUR) {
        BlurHdr& bh = *(BlurHdr*)blur_lds();
        sample_blur(rng, blur_ks, bh);
        sigma_out = bh.blur ? bh.sigma : 0.f;
      }
    } else {
      P.ci = 0; P.cj = 0; P.ch = H; P.cw = W; P.flip = 0; P.jitter = 0; P.gray = 0;
      P.fb = P.fc = P.fs = 1.f; P.fh = 0.f;
      for (int i = 0; i < 4; ++i) P.order[i] = i;
      if constexpr (BLUR) ((BlurHdr*)blur_lds())->blur = 0;
    }
    if (params_out) {
      float* po = params_out + ((size_t)blockIdx.y * n + b) * 16;
      po[0] = P.ci; po[1] = P.cj; po[2] = P.ch; po[3] = P.cw; po[4] = P.flip; po[5] = P.jitter;
      for (int i = 0; i < 4; ++i) po[6 + i] = P.order[i];
      po[10] = P.fb; po[11] = P.fc; po[12] = P.fs; po[13] = P.fh; po[14] = P.gray;
      po[15] = sigma_out;
    }
  }
  __syncthreads();
  const int npix = OH * OW;
  int kc = 4;  // position of contrast in the op order (4: none / jitter off)
  if (P.jitter)
    for (int i = 0; i < 4; ++i)
      if (P.order[i] == 1) kc = i;
  float mean = 0.f;
  if (kc < 4) {  // pass 1: mean luma of the image as contrast sees it
    long long s = 0;
    for (int p = threadIdx.x; p < npix; p += AUG_THREADS) {
      float r, g, bb;
      crop_pixel(P, img, W, OH, OW, p, r, g, bb);
      for (int i = 0; i < kc; ++i) pixel_op(P, P.order[i], r, g, bb);
      s += luma(r, g, bb);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    long long tot = 0;
    for (int w = 0; w < AUG_THREADS / 64; ++w) tot += red[w];
    mean = floorf((float)((double)tot / npix) + 0.5f);
  }
  const size_t obase = ((size_t)blockIdx.y * n + b) * npix;
  if constexpr (BLUR) {
    const BlurHdr& bh = *(const BlurHdr*)blur_lds();
    if (bh.blur) {  // per image: the whole block goes this way or none of it
      blur_bands(P, bh, img, W, OH, OW, Cpad, kc, mean, blur_ks, blur_band, blur_rows, out, obase);
      return;
    }
  }
  for (int p = threadIdx.x; p < npix; p += AUG_THREADS) {  // pass 2
    float r, g, bb;
    final_pixel(P, img, W, OH, OW, p, kc, mean, r, g, bb);
    store_pixel(out + (obase + p) * Cpad, Cpad, r, g, bb);
  }
}

bool large_output(int OH, int OW) { return OH * OW > AUG_THREADS * MAX_PIX_PER_THREAD; }

// rows of a blurred image that k_augment_large can stage (blur_bands: 7 bytes per pixel)
int blur_fit_rows(int OW) { return (BLUR_LDS_BYTES - BLUR_HDR_BYTES) / (7 * OW); }

}  // namespace

int augment_max_blur_kernel() { return AUG_MAX_BLUR_KS; }

// Output rows per band of a blurred image (the whole image where it fits; OH for the
// register-resident kernel, which stages whole images), 0: this size cannot be blurred.
int augment_blur_band(int OH, int OW, int ks) {
  if (ks < 3 || !(ks & 1) || ks > AUG_MAX_BLUR_KS || (ks >> 1) > (OH < OW ? OH : OW) - 1) return 0;
  if (!large_output(OH, OW)) return OH;
  const int fit = blur_fit_rows(OW);
  if (fit >= OH) return OH;
  return fit - (ks - 1) > 0 ? fit - (ks - 1) : 0;
}

void simclr_augment(const uint8_t* images, const int64_t* indices, int n, int views, int H, int W,
                    int OH, int OW, int Cpad, float strength, uint64_t seed, uint64_t counter,
                    int view_offset, int flags, uint16_t* out, float* params_out, int blur_kernel,
                    hipStream_t s) {
  const int band = blur_kernel ? augment_blur_band(OH, OW, blur_kernel) : 0;
  if (blur_kernel && (band <= 0 || !(flags & 1))) {  // the binding checks; never launch unchecked
    fprintf(stderr, "simclr_augment: unsupported blur_kernel %d for %dx%d\n", blur_kernel, OH, OW);
    abort();
  }
  if (large_output(OH, OW)) {  // two-pass kernel, any size
    if (blur_kernel) {
      const int rows = band == OH ? OH : band + blur_kernel - 1;
      const size_t lds = BLUR_HDR_BYTES + (size_t)rows * OW * 7;
      hipLaunchKernelGGL(k_augment_large<true>, dim3(n, views), dim3(AUG_THREADS), lds, s, images,
                         indices, n, H, W, OH, OW, Cpad, strength, seed, counter, view_offset,
                         flags, out, params_out, blur_kernel, band, rows);
    } else {
      hipLaunchKernelGGL(k_augment_large<false>, dim3(n, views), dim3(AUG_THREADS), 0, s, images,
                         indices, n, H, W, OH, OW, Cpad, strength, seed, counter, view_offset,
                         flags, out, params_out, 0, 0, 0);
    }
    HIP_CHECK_LAUNCH();
    return;
  }
  if (blur_kernel) {
    const size_t lds = BLUR_HDR_BYTES + (size_t)OH * OW * 2 * sizeof(float);
    hipLaunchKernelGGL(k_augment<true>, dim3(n, views), dim3(AUG_THREADS), lds, s, images, indices,
                       n, H, W, OH, OW, Cpad, strength, seed, counter, view_offset, flags, out,
                       params_out, blur_kernel);
  } else {
    hipLaunchKernelGGL(k_augment<false>, dim3(n, views), dim3(AUG_THREADS), 0, s, images, indices,
                       n, H, W, OH, OW, Cpad, strength, seed, counter, view_offset, flags, out,
                       params_out, 0);
  }
  HIP_CHECK_LAUNCH();
}
