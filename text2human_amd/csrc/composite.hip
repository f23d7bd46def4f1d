// Two-band compositing of an edited region back into the source photo (include/t2h_hip.h,
// t2h_composite_region_f32).  One workgroup = one 32 x 32 output tile of one image, all three
// channels.  A tile is classified from the keep mask alone: farther than r_lo from every edited cell -> the photo's
// pixels are copied (dec and LDS are never touched), wholly inside edited cells -> the decoder's pixels are copied,
// anything else stages the (32 + 2R)^2 halo of dec - p in LDS, one channel at a time, and blurs it there: horizontal
// pass into a second LDS buffer, vertical pass out of it.  The low band never reaches global memory.
#include "common.h"

namespace {

constexpr int CMP_T = 32;                         // tile edge (pixels)
constexpr int CMP_R_MAX = 32;                     // widest blur radius
// halo rows are laid out with the ODD stride 32 + 2R + 1: the horizontal pass has 8 lanes per row (4 outputs each)
// and 4 rows per 32-lane group, lane address = row * stride + 4 g + j -- an odd stride puts the 4 rows on the 4
// residues mod 4 that the 8 groups leave free, so a ds_read_b32 of the group touches 32 different banks
constexpr int CMP_STAGE = 13;                     // halo elements a thread stages per round (80 x 80 / 256 = 25: two rounds)
constexpr int CMP_CHUNK = 8;                      // taps per step of a blur pass

// the epilogue's formula (misc.hip, image_epilogue_kernel): ((x + 1) / 2).clamp(0, 1) in fp32
__device__ __forceinline__ float cmp_photo(float x, int is_signed) {
  if (!is_signed) return x;
  const float v = (x + 1.0f) / 2.0f;
  return fminf(fmaxf(v, 0.f), 1.f);
}

__device__ __forceinline__ unsigned cmp_u8(float v) {
  const float s = fminf(fmaxf(__fadd_rn(__fmul_rn(v, 255.0f), 0.5f), 0.f), 255.f);
  return (unsigned)(uint8_t)s;
}

// gap in pixels between pixel rows (columns) a0 .. a1 and b0 .. b1: 0 if they overlap, 1 if they touch
__device__ __forceinline__ int cmp_gap(int a0, int a1, int b0, int b1) { return max(0, max(b0 - a1, a0 - b1)); }

// Four neighbouring outputs of one blur pass on a sliding window: a[e] = sum over j < nt of tapbuf[j] src[(e + j) step],
// e = 0 .. 3, CMP_CHUNK taps at a time: the chunk's new values and its taps are read first -- independent LDS reads, all
// in flight together; one read per tap, each waited for, left a blended tile (and with it the launch) waiting on LDS
// latency -- then its 4 CMP_CHUNK fmas run, j ascending.  tapbuf holds zeros behind its nt taps up to a multiple of
// CMP_CHUNK, and a read past position `last` (>= nt + 3) goes to `last`, a float the caller keeps at zero: the tail of
// the last chunk adds 0 * 0.
__device__ __forceinline__ void cmp_pass4(const float* src, int step, int last, const float* tapbuf, int nt, float (&a)[4]) {
  float w[4 + CMP_CHUNK];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    w[e] = src[e * step];
    a[e] = 0.f;
  }
  for (int j0 = 0; j0 < nt; j0 += CMP_CHUNK) {
    float tp[CMP_CHUNK];
#pragma unroll
    for (int k = 0; k < CMP_CHUNK; ++k) {
      w[4 + k] = src[min(j0 + 4 + k, last) * step];
      tp[k] = tapbuf[j0 + k];
    }
#pragma unroll
    for (int k = 0; k < CMP_CHUNK; ++k)
#pragma unroll
      for (int e = 0; e < 4; ++e) a[e] = fmaf(tp[k], w[e + k], a[e]);
#pragma unroll
    for (int e = 0; e < 4; ++e) w[e] = w[CMP_CHUNK + e];
  }
}

__global__ __launch_bounds__(256) void composite_region_kernel(
    const float* __restrict__ dec, const float* __restrict__ photo, const uint8_t* __restrict__ keep,
    const float* __restrict__ taps, float* __restrict__ out, uint8_t* __restrict__ u8, int H, int W, int th, int tw,
    int cell, int r_hi, int r_lo, int R, int is_signed, int vec, int dbuf_floats) {
  // LDS is sized by the launch for this R (t2h_composite_region_f32): most tiles are copies that never touch it, and
  // what a workgroup reserves decides how many of them a CU holds
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* dbuf = smem;                                                   // halo of dec - p (first: the keep window)
  float* hbuf = smem + dbuf_floats;                                     // after the horizontal pass (+ a spare row)
  float* tapbuf = hbuf + (CMP_T + 2 * R + 1) * CMP_T;
  const int t = threadIdx.x, b = blockIdx.z;
  const int tx0 = blockIdx.x * CMP_T, ty0 = blockIdx.y * CMP_T;
  const int tx1 = min(tx0 + CMP_T, W) - 1, ty1 = min(ty0 + CMP_T, H) - 1;  // (the tile clipped to the image)
  const int64_t HW = (int64_t)H * W;
  const int64_t img0 = (int64_t)b * 3 * HW;
  const uint8_t* kb = keep + (int64_t)b * th * tw;

  // ---- the cells that can lie closer than r_lo to a pixel of the tile: rows wr0 .. wr1, columns wc0 .. wc1
  const int wr0 = max(ty0 - r_lo, 0) / cell, wr1 = min(ty1 + r_lo, H - 1) / cell;
  const int wc0 = max(tx0 - r_lo, 0) / cell, wc1 = min(tx1 + r_lo, W - 1) / cell;
  const int wcols = wc1 - wc0 + 1, wn = (wr1 - wr0 + 1) * wcols;
  // every wave classifies the tile on its own (its lanes share the cells, one vote each): no LDS, no barrier
  int near = 0, notin = 0;
  for (int i = t & 63; i < wn; i += 64) {
    const int r = wr0 + i / wcols, c = wc0 + i % wcols;
    const int g = max(cmp_gap(ty0, ty1, cell * r, cell * r + cell - 1), cmp_gap(tx0, tx1, cell * c, cell * c + cell - 1));
    const bool edited = kb[r * tw + c] == 0;
    near |= (edited && g < r_lo) ? 1 : 0;
    notin |= (!edited && g == 0) ? 1 : 0;
  }
  near = __any(near);
  notin = __any(notin);

  if (!near || !notin) {
    // ---- a copy: the photo's pixels (no pixel has d < r_lo) or the decoder's (every pixel has d == 0)
    const float* __restrict__ src = near ? dec : photo;
    const int xf = near ? 0 : is_signed;
    if (vec) {  // W % 4 == 0 and 16-byte aligned images: one f32x4 per channel, 12 bytes of uint8
      const int y = ty0 + (t >> 3), x = tx0 + 4 * (t & 7);
      if (y > ty1 || x > tx1) return;
      const int64_t o = img0 + (int64_t)y * W + x;
      f32x4 v[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) v[c] = *reinterpret_cast<const f32x4*>(src + o + c * HW);
#pragma unroll
      for (int c = 0; c < 3; ++c) {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[c][e] = cmp_photo(v[c][e], xf);
        *reinterpret_cast<f32x4*>(out + o + c * HW) = v[c];
      }
      if (u8) {
        unsigned wd[3] = {0u, 0u, 0u};
#pragma unroll
        for (int k = 0; k < 12; ++k) wd[k >> 2] |= cmp_u8(v[k % 3][k / 3]) << (8 * (k & 3));
        unsigned* q = reinterpret_cast<unsigned*>(u8 + (((int64_t)b * H + y) * W + x) * 3);
        q[0] = wd[0];
        q[1] = wd[1];
        q[2] = wd[2];
      }
      return;
    }
    const int x = tx0 + (t & 31);
    if (x > tx1) return;
    for (int y = ty0 + (t >> 5); y <= ty1; y += 8) {
      const int64_t o = img0 + (int64_t)y * W + x;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float v = cmp_photo(src[o + c * HW], xf);
        out[o + c * HW] = v;
        if (u8) u8[(((int64_t)b * H + y) * W + x) * 3 + c] = (uint8_t)cmp_u8(v);
      }
    }
    return;
  }

  // ---- a blended tile.  The keep window goes to LDS first (it borrows the halo buffer: wn <= 160 * 160 bytes)
  unsigned char* kwin = reinterpret_cast<unsigned char*>(dbuf);
  for (int i = t; i < wn; i += 256) kwin[i] = kb[(wr0 + i / wcols) * tw + wc0 + i % wcols];
  if (t < ((2 * R + CMP_CHUNK) & ~(CMP_CHUNK - 1))) tapbuf[t] = t < 2 * R + 1 ? taps[t] : 0.f;  // (zeros up to a whole chunk)
  __syncthreads();
  // thread -> column px, rows py0 .. py0 + 3 of the tile; d = min(Chebyshev distance to an edited cell, r_lo)
  const int lx = t & 31, ly0 = 4 * (t >> 5);
  const int px = tx0 + lx, py0 = ty0 + ly0;
  const int ncell = (r_lo + cell - 1) / cell;
  int d[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int y = py0 + e;
    int best = r_lo;
    if (y <= ty1 && px <= tx1) {
      const int cr = y / cell, cc = px / cell;
      for (int r = max(wr0, cr - ncell); r <= min(wr1, cr + ncell); ++r) {
        const int gy = cmp_gap(y, y, cell * r, cell * r + cell - 1);
        if (gy >= best) continue;
        for (int c = max(wc0, cc - ncell); c <= min(wc1, cc + ncell); ++c)
          if (kwin[(r - wr0) * wcols + (c - wc0)] == 0)
            best = min(best, max(gy, cmp_gap(px, px, cell * c, cell * c + cell - 1)));
      }
    }
    d[e] = best;
  }
  __syncthreads();  // (the window is dead: the halo may overwrite it)

  const int hr = CMP_T + 2 * R, hs = hr + 1, nt = 2 * R + 1;
  // the padding float of every halo row and the spare row behind the horizontal pass's buffer: what the last chunk of
  // a pass reads beyond its taps (cmp_pass4); nothing below writes them again
  if (t < hr) dbuf[t * hs + hr] = 0.f;
  if (t < CMP_T) hbuf[hr * CMP_T + t] = 0.f;
  float o[3][4];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float* __restrict__ dc = dec + img0 + c * HW;
    const float* __restrict__ pc = photo + img0 + c * HW;
    // halo of diff = dec - p, coordinates clamped to the image (replicate)
    // (CMP_STAGE elements per thread and round: their 2 CMP_STAGE loads are issued before the first is used -- a
    // blended tile is alone with its latencies, and the slowest tile is the launch's duration)
    for (int i0 = t; i0 < hr * hr; i0 += 256 * CMP_STAGE) {
      float dv[CMP_STAGE], pv[CMP_STAGE];
      int at[CMP_STAGE];
#pragma unroll
      for (int u = 0; u < CMP_STAGE; ++u) {
        const int i = min(i0 + 256 * u, hr * hr - 1);  // (past the end: the last element once more, not stored)
        const int r = i / hr, q = i - r * hr;
        const int y = min(max(ty0 - R + r, 0), H - 1), x = min(max(tx0 - R + q, 0), W - 1);
        const int64_t g = (int64_t)y * W + x;
        dv[u] = dc[g];
        pv[u] = pc[g];
        at[u] = i0 + 256 * u < hr * hr ? r * hs + q : -1;
      }
#pragma unroll
      for (int u = 0; u < CMP_STAGE; ++u)
        if (at[u] >= 0) dbuf[at[u]] = dv[u] - cmp_photo(pv[u], is_signed);
    }
    __syncthreads();  // (also: every thread is past the previous channel's vertical pass, hbuf is free)
    // horizontal pass: 4 consecutive outputs per thread on a sliding window
    for (int i = t; i < hr * (CMP_T / 4); i += 256) {
      const int r = i >> 3, x0 = (i & 7) * 4;
      float a[4];
      cmp_pass4(dbuf + r * hs + x0, 1, hr - x0, tapbuf, nt, a);
      const f32x4 av = {a[0], a[1], a[2], a[3]};
      *reinterpret_cast<f32x4*>(hbuf + r * CMP_T + x0) = av;
    }
    __syncthreads();
    // vertical pass of the thread's 4 rows, then the combine
    {
      float low[4];
      cmp_pass4(hbuf + ly0 * CMP_T + lx, CMP_T, hr - ly0, tapbuf, nt, low);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int y = py0 + e;
        float v = 0.f;
        if (y <= ty1 && px <= tx1) {
          const int64_t g = (int64_t)y * W + px;
          const float dv = dc[g], pv = cmp_photo(pc[g], is_signed);
          if (d[e] == 0) {
            v = dv;
          } else if (d[e] >= r_lo) {
            v = pv;
          } else {
            const float df = dv - pv;
            const float wl = 1.0f - (float)d[e] / (float)r_lo;
            const float wh = fmaxf(0.f, 1.0f - (float)d[e] / (float)r_hi);
            v = fminf(fmaxf(pv + wl * low[e] + wh * (df - low[e]), 0.f), 1.f);
          }
        }
        o[c][e] = v;
      }
    }
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int y = py0 + e;
    if (y > ty1 || px > tx1) continue;
    const int64_t g = img0 + (int64_t)y * W + px;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      out[g + c * HW] = o[c][e];
      if (u8) u8[(((int64_t)b * H + y) * W + px) * 3 + c] = (uint8_t)cmp_u8(o[c][e]);
    }
  }
}

}  // namespace

extern "C" int t2h_composite_region_f32(const float* dec, const float* photo, const uint8_t* keep, const float* taps,
                                        float* out, uint8_t* out_u8, int32_t B, int32_t H, int32_t W, int32_t th,
                                        int32_t tw, int32_t r_hi, int32_t r_lo, int32_t R, int32_t photo_signed,
                                        void* stream) {
  T2H_REQUIRE(dec && photo && keep && taps && out, "t2h_composite_region_f32: NULL pointer");
  T2H_REQUIRE(out != dec && out != photo, "t2h_composite_region_f32: out must not alias dec or photo");
  T2H_REQUIRE(B > 0 && B <= 65535 && H > 0 && W > 0 && th > 0 && tw > 0 && (int64_t)H * W < (int64_t)1 << 31,
              "t2h_composite_region_f32: bad shape (B %d, H %d, W %d, th %d, tw %d)", B, H, W, th, tw);
  T2H_REQUIRE(H % th == 0 && W % tw == 0 && H / th == W / tw,
              "t2h_composite_region_f32: H x W (%d x %d) must be the same whole multiple of th x tw (%d x %d)", H, W, th,
              tw);
  T2H_REQUIRE(r_hi >= 1 && r_hi <= r_lo && r_lo <= 64,
              "t2h_composite_region_f32: need 1 <= r_hi <= r_lo <= 64, got r_hi %d, r_lo %d", r_hi, r_lo);
  T2H_REQUIRE(R >= 0 && R <= CMP_R_MAX, "t2h_composite_region_f32: need 0 <= R <= 32 (taps [2R + 1]), got %d", R);
  const int vec = W % 4 == 0 && t2h_aligned16(dec) && t2h_aligned16(photo) && t2h_aligned16(out) &&
                  (reinterpret_cast<uintptr_t>(out_u8) & 3u) == 0;
  // LDS: the halo (rows of odd stride 32 + 2R + 1) -- or the keep window it lends its place to first, at most
  // ((32 + 2 r_lo) / cell + 2)^2 bytes -- then (32 + 2R + 1) x 32 floats of the horizontal pass, then the taps (padded
  // with zeros to a whole chunk)
  const int cell = H / th, hr = CMP_T + 2 * R, wside = (CMP_T + 2 * r_lo) / cell + 2;
  const int dbuf_floats = ((hr * (hr + 1) > (wside * wside + 3) / 4 ? hr * (hr + 1) : (wside * wside + 3) / 4) + 3) & ~3;
  const size_t lds_bytes = sizeof(float) * ((size_t)dbuf_floats + (hr + 1) * CMP_T + ((2 * R + CMP_CHUNK) & ~(CMP_CHUNK - 1)));
  hipLaunchKernelGGL(composite_region_kernel, dim3((W + CMP_T - 1) / CMP_T, (H + CMP_T - 1) / CMP_T, B), dim3(256),
                     lds_bytes, static_cast<hipStream_t>(stream), dec, photo, keep, taps, out, out_u8, H, W, th, tw, cell,
                     r_hi, r_lo, R, photo_signed != 0, vec, dbuf_floats);
  T2H_CHECK_LAUNCH("t2h_composite_region_f32");
  return T2H_OK;
}
