// Garment colour control in image space (include/t2h_hip.h, t2h_region_color_stats / t2h_recolor_region_f32;
// DESIGN.md 4.6l).  Two kernels share one colour transform (rc_yuv / rc_rgb) and one membership rule (rc_code,
// t2h_region_keep's mode 2):
//   statistics: one workgroup per (image, stripe of RC_STRIPE rows) sums Y / U / V and their squares over the members
//               of every group in f64 -- per lane in ascending address order, a fixed butterfly over the wave, the four
//               waves in ascending order -- into one partial row per (stripe, group); a second, tiny launch adds the
//               stripes in ascending order.  No atomics on floating-point numbers: the order is fixed;
//   apply:      one workgroup per 32 x 32 tile of one image.  The membership codes of the (32 + 2f)^2 halo go to LDS,
//               one byte per pixel; the tent filter runs on integers, all four groups at once in the bytes of one word:
//               a horizontal pass into LDS (sums <= (f + 1)^2 = 81 per byte), then a vertical pass in two words of
//               16-bit fields (sums <= (f + 1)^4 = 6561).  A tile without a member in its halo copies p, a tile whose
//               halo is one group skips the passes (N = (f + 1)^4); both go through the same per-pixel function as the
//               general path.
#include "common.h"

namespace {

constexpr int RC_T = 32;                  // tile edge (pixels)
constexpr int RC_F_MAX = 8;               // widest feather
constexpr int RC_HS = RC_T + 2 * RC_F_MAX;  // halo row stride in bytes (48: a row's words stay aligned)
constexpr int RC_G_MAX = 4;
constexpr int RC_STRIPE = 16;             // rows of a statistics stripe (ops.RECOLOR_STRIPE)
constexpr unsigned RC_NONE = 0xffu;       // membership code of a pixel outside every (active) group

struct rc_bits {
  uint64_t g[RC_G_MAX];
};

// the epilogue's formula (misc.hip, image_epilogue_kernel): ((x + 1) / 2).clamp(0, 1) in fp32
__device__ __forceinline__ float rc_photo(float x, int is_signed) {
  if (!is_signed) return x;
  const float v = (x + 1.0f) / 2.0f;
  return fminf(fmaxf(v, 0.f), 1.f);
}

__device__ __forceinline__ unsigned rc_u8(float v) {
  const float s = fminf(fmaxf(__fadd_rn(__fmul_rn(v, 255.0f), 0.5f), 0.f), 255.f);
  return (unsigned)(uint8_t)s;
}

// The colour space, fp32, shared by both kernels: Y = 0.299 R + 0.587 G + 0.114 B, U = B - Y, V = R - Y.  Every
// operation is written out (fmaf / __fmul_rn / __fadd_rn): the compiler contracts nothing, every path of every kernel
// gives the same bits for the same pixel.
__device__ __forceinline__ void rc_yuv(float r, float g, float b, float& Y, float& U, float& V) {
  Y = fmaf(0.114f, b, fmaf(0.587f, g, __fmul_rn(0.299f, r)));
  U = __fadd_rn(b, -Y);
  V = __fadd_rn(r, -Y);
}
// the inverse: R = Y + V, B = Y + U, G = Y - (0.299 V + 0.114 U) / 0.587
__device__ __forceinline__ void rc_rgb(float Y, float U, float V, float& r, float& g, float& b) {
  r = __fadd_rn(Y, V);
  b = __fadd_rn(Y, U);
  g = __fadd_rn(Y, -(fmaf(0.114f, U, __fmul_rn(0.299f, V)) / 0.587f));
}

// t2h_region_keep's mode 2 (sampler.hip, region_keep_kernel): a float label is a member of the group whose bit
// (int)v is set iff 0 <= v < 64 and v is a whole number; anything else (negative, >= 64, fractional, NaN, inf) is in
// no group.  -> the group's index, or RC_NONE.  (The groups of a call are disjoint: at most one matches.)
__device__ __forceinline__ unsigned rc_code(float v, const rc_bits& bits, int G) {
  if (!(v >= 0.f && v < 64.f)) return RC_NONE;
  const int l = (int)v;
  if ((float)l != v) return RC_NONE;
  unsigned code = RC_NONE;
#pragma unroll
  for (int g = RC_G_MAX - 1; g >= 0; --g)
    if (g < G && ((bits.g[g] >> l) & 1ull)) code = (unsigned)g;
  return code;
}

// ---------------------------------------------------------------------------------------------------- statistics
// partial[b][stripe][g][8] = {n, sum Y, sum U, sum V, sum Y^2, sum U^2, sum V^2, 0} over the members of group g in the
// stripe's rows.  Lane t owns the pixel quads t, t + 256, ... of the stripe (4 consecutive pixels each, in address
// order) whether they are loaded 16 bytes at a time or one by one: the order of the sums does not depend on alignment.
__global__ __launch_bounds__(256) void region_color_partial_kernel(const float* __restrict__ img,
                                                                   const float* __restrict__ segm, rc_bits bits, int G,
                                                                   int H, int W, int is_signed, int vec,
                                                                   double* __restrict__ partial) {
  __shared__ double red[4][RC_G_MAX * 8];
  const int t = threadIdx.x, b = blockIdx.y, stripe = blockIdx.x;
  const int64_t HW = (int64_t)H * W;
  const float* __restrict__ ib = img + (int64_t)b * 3 * HW;
  const float* __restrict__ sb = segm + (int64_t)b * HW;
  const int64_t p0 = (int64_t)stripe * RC_STRIPE * W;
  const int64_t p1 = min(p0 + (int64_t)RC_STRIPE * W, HW);  // (the last stripe may be short)
  double acc[RC_G_MAX][6];
  int cnt[RC_G_MAX];
#pragma unroll
  for (int g = 0; g < RC_G_MAX; ++g) {
    cnt[g] = 0;
#pragma unroll
    for (int k = 0; k < 6; ++k) acc[g][k] = 0.0;
  }
  for (int64_t q = p0 + 4 * (int64_t)t; q < p1; q += 4 * 256) {
    float s[4], c[3][4];
    if (vec) {  // (W % 4 == 0: a quad never leaves the stripe)
      const f32x4 sv = *reinterpret_cast<const f32x4*>(sb + q);
      f32x4 cv[3];
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) cv[ch] = *reinterpret_cast<const f32x4*>(ib + ch * HW + q);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        s[e] = sv[e];
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) c[ch][e] = cv[ch][e];
      }
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int64_t i = min(q + e, p1 - 1);  // (past the end: the last pixel once more, not counted)
        s[e] = q + e < p1 ? sb[i] : -1.f;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) c[ch][e] = ib[ch * HW + i];
      }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const unsigned code = rc_code(s[e], bits, G);
      if (code == RC_NONE) continue;
      float Y, U, V;
      rc_yuv(rc_photo(c[0][e], is_signed), rc_photo(c[1][e], is_signed), rc_photo(c[2][e], is_signed), Y, U, V);
      const double dY = (double)Y, dU = (double)U, dV = (double)V;
#pragma unroll
      for (int g = 0; g < RC_G_MAX; ++g)
        if (code == (unsigned)g) {
          cnt[g] += 1;
          acc[g][0] += dY;
          acc[g][1] += dU;
          acc[g][2] += dV;
          acc[g][3] += dY * dY;
          acc[g][4] += dU * dU;
          acc[g][5] += dV * dV;
        }
    }
  }
  // the wave's butterfly (the same pairs in the same order on every run), then the four waves in ascending order
#pragma unroll
  for (int g = 0; g < RC_G_MAX; ++g) {
    if (g >= G) continue;  // (uniform)
    int n = cnt[g];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
    double v[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) v[k] = wave_sum_d(acc[g][k]);
    if ((t & 63) == 0) {
      red[t >> 6][g * 8] = (double)n;
#pragma unroll
      for (int k = 0; k < 6; ++k) red[t >> 6][g * 8 + 1 + k] = v[k];
      red[t >> 6][g * 8 + 7] = 0.0;
    }
  }
  __syncthreads();
  if (t < G * 8)
    partial[(((int64_t)b * gridDim.x + stripe) * G) * 8 + t] = ((red[0][t] + red[1][t]) + red[2][t]) + red[3][t];
}

// stats[b][g][8] = {n, mY, mU, mV, sY, sU, sV, 0}: the stripes added in ascending order, one workgroup per image
__global__ __launch_bounds__(64) void region_color_finalize_kernel(const double* __restrict__ partial, int G, int S,
                                                                 double* __restrict__ stats) {
  __shared__ double sum[RC_G_MAX * 8];
  const int t = threadIdx.x, b = blockIdx.x;
  if (t < G * 8) {
    double a = 0.0;
    for (int s = 0; s < S; ++s) a += partial[(((int64_t)b * S + s) * G) * 8 + t];
    sum[t] = a;
  }
  __syncthreads();
  if (t < G * 8) {
    const int g = t >> 3, k = t & 7;
    const double n = sum[g * 8];
    double r = 0.0;
    if (n > 0.0 && k < 7) {
      if (k == 0) {
        r = n;
      } else {
        const int c = (k - 1) % 3;
        const double m = sum[g * 8 + 1 + c] / n;
        r = k <= 3 ? m : sqrt(fmax(0.0, sum[g * 8 + 4 + c] / n - m * m));
      }
    }
    stats[((int64_t)b * G) * 8 + t] = r;
  }
}

// --------------------------------------------------------------------------------------------------------- apply
// per-group constants, formed in f64 from the two statistics rows and rounded once to fp32
struct rc_consts {
  float gain[3];  // clamp(t.s_c / s.s_c, 1 / gain_max, gain_max), or 1 (c = Y, U, V)
  float sm[3];    // s.mY, s.mU, s.mV
  float dY;       // luma (t.mY - s.mY)
  float tmU, tmV;
};

// out = p (its bits) where no active group has weight; elsewhere clamp(p + sum_g alpha_g (T_g(p) - p), 0, 1), g
// ascending, alpha_g = N_g / D.  The one per-pixel function of every path.
__device__ __forceinline__ void rc_pixel(const float (&p)[3], const int (&N)[RC_G_MAX], float D, const rc_consts* kc, int G,
                                         float (&o)[3]) {
  o[0] = p[0];
  o[1] = p[1];
  o[2] = p[2];
  if ((N[0] | N[1] | N[2] | N[3]) == 0) return;
  float Y, U, V;
  rc_yuv(p[0], p[1], p[2], Y, U, V);
  float a[3] = {0.f, 0.f, 0.f};
#pragma unroll
  for (int g = 0; g < RC_G_MAX; ++g) {
    if (g >= G || N[g] == 0) continue;
    const rc_consts k = kc[g];
    const float alpha = (float)N[g] / D;
    const float Y2 = __fadd_rn(fmaf(k.gain[0], __fadd_rn(Y, -k.sm[0]), k.sm[0]), k.dY);
    const float U2 = fmaf(k.gain[1], __fadd_rn(U, -k.sm[1]), k.tmU);
    const float V2 = fmaf(k.gain[2], __fadd_rn(V, -k.sm[2]), k.tmV);
    float T[3];
    rc_rgb(Y2, U2, V2, T[0], T[1], T[2]);
#pragma unroll
    for (int c = 0; c < 3; ++c) a[c] = fmaf(alpha, __fadd_rn(T[c], -p[c]), a[c]);
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) o[c] = fminf(fmaxf(__fadd_rn(p[c], a[c]), 0.f), 1.f);
}

__global__ __launch_bounds__(256) void recolor_region_kernel(const float* __restrict__ img, const float* __restrict__ segm,
                                                             rc_bits bits, int G, const double* __restrict__ src_stats,
                                                             const double* __restrict__ dst_stats, float luma,
                                                             float gain_max, int f, float* __restrict__ out,
                                                             uint8_t* __restrict__ u8, int H, int W, int is_signed,
                                                             int vec) {
  __shared__ __attribute__((aligned(16))) unsigned char s_code[RC_HS * RC_HS];  // membership codes of the halo
  __shared__ __attribute__((aligned(16))) unsigned s_h[RC_HS * RC_T];           // horizontal pass, 4 groups x 8 bits
  __shared__ rc_consts s_k[RC_G_MAX];
  __shared__ int s_active[RC_G_MAX];
  __shared__ int s_seen;
  const int t = threadIdx.x, b = blockIdx.z;
  const int tx0 = blockIdx.x * RC_T, ty0 = blockIdx.y * RC_T;
  const int tx1 = min(tx0 + RC_T, W) - 1, ty1 = min(ty0 + RC_T, H) - 1;  // (the tile clipped to the image)
  const int64_t HW = (int64_t)H * W;
  const int64_t img0 = (int64_t)b * 3 * HW;
  const float* __restrict__ sb = segm + (int64_t)b * HW;

  // ---- the groups' constants, once per workgroup
  if (t < RC_G_MAX) {
    int active = 0;
    if (t < G) {
      const double* s = src_stats + ((int64_t)b * G + t) * 8;
      const double* d = dst_stats + ((int64_t)b * G + t) * 8;
      active = (s[0] > 0.0 && d[0] > 0.0) ? 1 : 0;
      const double gm = (double)gain_max;
      rc_consts k;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        double gn = 1.0;
        if (s[4 + c] > 1e-6 && d[4 + c] > 0.0) gn = fmin(fmax(d[4 + c] / s[4 + c], 1.0 / gm), gm);
        k.gain[c] = (float)gn;
        k.sm[c] = (float)s[1 + c];
      }
      k.dY = (float)((double)luma * (d[1] - s[1]));
      k.tmU = (float)d[2];
      k.tmV = (float)d[3];
      s_k[t] = k;
    }
    s_active[t] = active;
    if (t == 0) s_seen = 0;
  }
  __syncthreads();

  // ---- membership codes of the (32 + 2f)^2 halo, coordinates clamped to the image (replicate); a member of an
  // inactive group counts as no member.  seen: bit g = a member of active group g, bit 4 = anything else
  const int hs = RC_T + 2 * f;
  int seen = 0;
  for (int i = t; i < hs * hs; i += 256) {
    const int r = i / hs, q = i - r * hs;
    const int y = min(max(ty0 - f + r, 0), H - 1), x = min(max(tx0 - f + q, 0), W - 1);
    unsigned code = rc_code(sb[(int64_t)y * W + x], bits, G);
    if (code != RC_NONE && !s_active[code]) code = RC_NONE;
    s_code[r * RC_HS + q] = (unsigned char)code;
    seen |= code == RC_NONE ? 16 : 1 << code;
  }
  atomicOr(&s_seen, seen);
  __syncthreads();
  seen = s_seen;

  // thread -> row ly of the tile, columns x0 .. x0 + 3
  const int ly = t >> 3, x0 = 4 * (t & 7);
  const int y = ty0 + ly, px = tx0 + x0;
  const int D = (f + 1) * (f + 1) * (f + 1) * (f + 1);
  int N[4][RC_G_MAX];
#pragma unroll
  for (int e = 0; e < 4; ++e)
#pragma unroll
    for (int g = 0; g < RC_G_MAX; ++g) N[e][g] = 0;
  if ((seen & 15) != 0 && (seen & (seen - 1)) == 0) {
    // ---- the whole halo is one active group: every window is all members, N = (f + 1)^4
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
      for (int g = 0; g < RC_G_MAX; ++g) N[e][g] = (seen >> g) & 1 ? D : 0;
  } else if ((seen & 15) != 0) {
    // ---- horizontal pass: h[r][x] = sum_j (f + 1 - |j|) m_g(r, x + j), group g in byte g (<= 81 each)
    int wt[4 + 2 * RC_F_MAX];
#pragma unroll
    for (int k = 0; k < 4 + 2 * RC_F_MAX; ++k) wt[k] = max(0, f + 1 - abs(k - f));  // (0 beyond the 2f + 1 taps)
    for (int i = t; i < hs * (RC_T / 4); i += 256) {
      const int r = i >> 3, c0 = (i & 7) * 4;
      const unsigned* row = reinterpret_cast<const unsigned*>(s_code + r * RC_HS + c0);
      unsigned w[(4 + 2 * RC_F_MAX) / 4];
#pragma unroll
      for (int k = 0; k < (4 + 2 * RC_F_MAX) / 4; ++k) w[k] = row[k];  // (c0 + 20 <= 48: inside the row)
      unsigned h[4] = {0u, 0u, 0u, 0u};
#pragma unroll
      for (int k = 0; k < 4 + 2 * RC_F_MAX; ++k) {
        const unsigned code = (w[k >> 2] >> (8 * (k & 3))) & 0xffu;
        const unsigned one = code < (unsigned)RC_G_MAX ? 1u << (8 * code) : 0u;  // (bytes beyond the halo: weight 0)
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (k - e >= 0 && k - e <= 2 * RC_F_MAX) h[e] += (unsigned)wt[k - e] * one;
      }
      typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
      const u32x4 hv = {h[0], h[1], h[2], h[3]};
      *reinterpret_cast<u32x4*>(s_h + r * RC_T + c0) = hv;
    }
    __syncthreads();
    // vertical pass: N_g = sum_i (f + 1 - |i|) h_g[ly + i], groups 0 / 2 and 1 / 3 in the 16-bit halves of two words
    {
      typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
      unsigned lo[4] = {0u, 0u, 0u, 0u}, hi[4] = {0u, 0u, 0u, 0u};
      for (int i = 0; i <= 2 * f; ++i) {
        const unsigned wi = (unsigned)(f + 1 - abs(i - f));
        const u32x4 hv = *reinterpret_cast<const u32x4*>(s_h + (ly + i) * RC_T + x0);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          lo[e] += wi * (hv[e] & 0x00ff00ffu);
          hi[e] += wi * ((hv[e] >> 8) & 0x00ff00ffu);
        }
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        N[e][0] = (int)(lo[e] & 0xffffu);
        N[e][1] = (int)(hi[e] & 0xffffu);
        N[e][2] = (int)(lo[e] >> 16);
        N[e][3] = (int)(hi[e] >> 16);
      }
    }
  }
  // (no member of an active group in the halo: N stays 0 and every pixel is p)

  // ---- the tile's pixels: 16-byte accesses where W % 4 == 0 and the images are aligned, one by one otherwise
  if (y > ty1 || px > tx1) return;
  const int64_t o0 = img0 + (int64_t)y * W + px;
  float p[3][4], o[3][4];
  if (vec) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(img + o0 + c * HW);
#pragma unroll
      for (int e = 0; e < 4; ++e) p[c][e] = v[e];
    }
  } else {
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
      for (int e = 0; e < 4; ++e) p[c][e] = img[o0 + c * HW + min(e, tx1 - px)];
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const float pe[3] = {rc_photo(p[0][e], is_signed), rc_photo(p[1][e], is_signed), rc_photo(p[2][e], is_signed)};
    float oe[3];
    rc_pixel(pe, N[e], (float)D, s_k, G, oe);
    o[0][e] = oe[0];
    o[1][e] = oe[1];
    o[2][e] = oe[2];
  }
  if (vec) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const f32x4 v = {o[c][0], o[c][1], o[c][2], o[c][3]};
      *reinterpret_cast<f32x4*>(out + o0 + c * HW) = v;
    }
    if (u8) {
      unsigned wd[3] = {0u, 0u, 0u};
#pragma unroll
      for (int k = 0; k < 12; ++k) wd[k >> 2] |= rc_u8(o[k % 3][k / 3]) << (8 * (k & 3));
      unsigned* q = reinterpret_cast<unsigned*>(u8 + (((int64_t)b * H + y) * W + px) * 3);
      q[0] = wd[0];
      q[1] = wd[1];
      q[2] = wd[2];
    }
    return;
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    if (px + e > tx1) continue;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      out[o0 + c * HW + e] = o[c][e];
      if (u8) u8[(((int64_t)b * H + y) * W + px + e) * 3 + c] = (uint8_t)rc_u8(o[c][e]);
    }
  }
}

// shared argument checks -> the groups' bit sets by value
int rc_groups(const char* name, const uint64_t* label_bits, int32_t G, rc_bits* bits) {
  T2H_REQUIRE(G >= 1 && G <= RC_G_MAX, "%s: need 1 <= G <= 4 groups, got %d", name, G);
  T2H_REQUIRE(label_bits != nullptr, "%s: NULL pointer", name);
  uint64_t all = 0;
  for (int g = 0; g < RC_G_MAX; ++g) {
    bits->g[g] = g < G ? label_bits[g] : 0;
    T2H_REQUIRE((all & bits->g[g]) == 0, "%s: the groups must be disjoint (group %d shares a label with an earlier one)",
                name, g);
    all |= bits->g[g];
  }
  return T2H_OK;
}

}  // namespace

extern "C" int t2h_region_color_stats(const float* img, int32_t img_signed, const float* segm, const uint64_t* label_bits,
                                      int32_t G, int32_t B, int32_t H, int32_t W, double* partial, double* stats,
                                      void* stream) {
  T2H_REQUIRE(img && segm && label_bits && partial && stats, "t2h_region_color_stats: NULL pointer");
  T2H_REQUIRE(B > 0 && B <= 65535 && H > 0 && W > 0 && (int64_t)H * W < (int64_t)1 << 31,
              "t2h_region_color_stats: bad shape (B %d, H %d, W %d)", B, H, W);
  rc_bits bits;
  if (rc_groups("t2h_region_color_stats", label_bits, G, &bits) != T2H_OK) return T2H_ERR_INVALID;
  const int S = (H + RC_STRIPE - 1) / RC_STRIPE;
  const int vec = W % 4 == 0 && t2h_aligned16(img) && t2h_aligned16(segm);
  hipLaunchKernelGGL(region_color_partial_kernel, dim3(S, B), dim3(256), 0, static_cast<hipStream_t>(stream), img, segm,
                     bits, G, H, W, img_signed != 0, vec, partial);
  T2H_CHECK_LAUNCH("t2h_region_color_stats");
  hipLaunchKernelGGL(region_color_finalize_kernel, dim3(B), dim3(64), 0, static_cast<hipStream_t>(stream), partial, G, S,
                     stats);
  T2H_CHECK_LAUNCH("t2h_region_color_stats (finalize)");
  return T2H_OK;
}

extern "C" int t2h_recolor_region_f32(const float* img, int32_t img_signed, const float* segm, const uint64_t* label_bits,
                                      int32_t G, const double* src_stats, const double* dst_stats, float luma,
                                      float gain_max, int32_t feather, float* out, uint8_t* out_u8, int32_t B, int32_t H,
                                      int32_t W, void* stream) {
  T2H_REQUIRE(img && segm && label_bits && src_stats && dst_stats && out, "t2h_recolor_region_f32: NULL pointer");
  T2H_REQUIRE(out != img, "t2h_recolor_region_f32: out must not alias img");
  T2H_REQUIRE(B > 0 && B <= 65535 && H > 0 && W > 0 && (int64_t)H * W < (int64_t)1 << 31,
              "t2h_recolor_region_f32: bad shape (B %d, H %d, W %d)", B, H, W);
  rc_bits bits;
  if (rc_groups("t2h_recolor_region_f32", label_bits, G, &bits) != T2H_OK) return T2H_ERR_INVALID;
  T2H_REQUIRE(feather >= 0 && feather <= RC_F_MAX, "t2h_recolor_region_f32: need 0 <= feather <= 8, got %d", feather);
  T2H_REQUIRE(luma >= 0.f && luma <= 1.f, "t2h_recolor_region_f32: need 0 <= luma <= 1, got %g", (double)luma);
  T2H_REQUIRE(gain_max >= 1.f && gain_max <= 16.f, "t2h_recolor_region_f32: need 1 <= gain_max <= 16, got %g",
              (double)gain_max);
  const int vec = W % 4 == 0 && t2h_aligned16(img) && t2h_aligned16(out) && (reinterpret_cast<uintptr_t>(out_u8) & 3u) == 0;
  hipLaunchKernelGGL(recolor_region_kernel, dim3((W + RC_T - 1) / RC_T, (H + RC_T - 1) / RC_T, B), dim3(256), 0,
                     static_cast<hipStream_t>(stream), img, segm, bits, G, src_stats, dst_stats, luma, gain_max, feather, out,
                     out_u8, H, W, img_signed != 0, vec);
  T2H_CHECK_LAUNCH("t2h_recolor_region_f32");
  return T2H_OK;
}
