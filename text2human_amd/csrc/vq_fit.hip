// All-codebook fit of latent rows: for every row and every texture codebook the least expanded
// distance min_j ((sum z^2 + sum e_j^2) - 2 z.e_j) and the first j that attains it -- a [n, 256] x [n_books n_e, 256]^T
// contraction on v_mfma_f32_32x32x2_f32 whose [n, n_books n_e] result is never written: the running (min, argmin) of
// a row lives in the registers of the lanes that own the row's accumulator elements -- and the per-region vote that
// turns the per-row minima into the three texture attributes of an image.
//
// Fit kernel, modelled on gemm.hip's staged loop:
//   * a workgroup = 4 waves owns BM rows x ONE book; it walks the book's codes in tiles of BN = 128 and K in tiles of
//     BK = 32.  Wave tile 32 rows x (128 / WARPS_N) codes: (BM, WARPS_N) = (128, 1), (64, 2) or (32, 4) -- the small
//     row tiles fill the chip at small n (one image = 512 rows x 18 books is 288 workgroups of 32 rows);
//   * global -> registers -> LDS, rows padded to BK + 4 floats, two LDS buffers, ONE barrier per K tile; the MFMA k
//     pair of step s is (s, BK/2 + s) of the tile, K tiles ascending: the k order of a (row, code) dot product is
//     fixed and the same in every tile shape, so a row's outputs are a function of the row and the books alone;
//   * sum e_j^2 comes from the very registers that stage the code tile (an fma chain per thread over the 8 K tiles,
//     then a fixed 8-lane butterfly), sum z^2 from a wave reduction of the row at the start;
//   * after a code tile's 8 K tiles every lane folds its 16 x TN accumulator elements into 16 (min, argmin) pairs
//     (codes ascending, strict <: the first minimum stays); lanes, then waves, are combined ONCE at the end with ties
//     going to the lower index.  A distance that is NaN or +inf never wins: a row without a comparable code keeps
//     (+inf, -1).
#include "common.h"

namespace {

constexpr int FIT_D = 256;
constexpr int FIT_BN = 128;
constexpr int FIT_BK = 32;
constexpr int FIT_NT = 256;

// (value, index) with the lower index winning a tie; index -1 only ever comes with +inf
__device__ __forceinline__ void fit_take(float& b, int& bj, float ob, int oj) {
  if (ob < b || (ob == b && oj < bj)) {
    b = ob;
    bj = oj;
  }
}

template <int WARPS_M, int WARPS_N>
__global__ __launch_bounds__(FIT_NT) void vq_fit_kernel(const float* __restrict__ z, const float* __restrict__ books,
                                                        float* __restrict__ dmin, int32_t* __restrict__ jmin, int n,
                                                        int n_books, int n_e) {
  static_assert(WARPS_M * WARPS_N == 4, "four waves");
  constexpr int BM = 32 * WARPS_M, BN = FIT_BN, BK = FIT_BK, D = FIT_D;
  constexpr int LDS_LD = BK + 4;
  constexpr int KQ = BK / 4;        // float4 per tile row
  constexpr int RPP = FIT_NT / KQ;  // tile rows staged per pass (32)
  constexpr int A_F4 = BM / RPP, B_F4 = BN / RPP;
  constexpr int WN = BN / WARPS_N, TN = WN / 32;
  constexpr int NKT = D / BK;       // K tiles per code tile (8)
  constexpr int STEPS = BK / 2;     // MFMA k-steps per K tile
  constexpr int NPIECE = A_F4 + B_F4;
  static_assert(2 * NPIECE <= STEPS, "one staging piece per MFMA step");
  constexpr int FIRST = STEPS - 2 * NPIECE;

  __shared__ __attribute__((aligned(16))) float smem[2 * (BM + BN) * LDS_LD];
  __shared__ float zz_s[BM];
  __shared__ float ee_s[2][BN];
  __shared__ float red_v[WARPS_N][BM];
  __shared__ int red_j[WARPS_N][BM];
  float* const As = smem;
  float* const Bs = smem + 2 * BM * LDS_LD;

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int l31 = lane & 31, hh = lane >> 5;
  const int wm = wave / WARPS_N, wn = wave % WARPS_N;
  const int wm0 = wm * 32, wn0 = wn * WN;
  // XCD-aware mapping as in gemm.hip: workgroup b runs on XCD b % 8; every XCD gets a contiguous range of the
  // (book, row tile) sequence, so the workgroups that share an L2 share a book
  const int nrt = (n + BM - 1) / BM;
  int book, m0;
  {
    const int total = nrt * n_books, b = blockIdx.x;
    const int xcd = b & 7, slot = b >> 3, q = total >> 3, r = total & 7;
    const int lin = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + slot;
    book = lin / nrt;
    m0 = (lin - book * nrt) * BM;
  }
  const float* __restrict__ Bg = books + (int64_t)book * n_e * D;
  const int n_ct = (n_e + BN - 1) / BN;
  const int G = n_ct * NKT;  // (code tile, K tile) pairs, walked in this order

  // ---- sum z^2 of this workgroup's rows: one row per wave at a time, one float4 per lane
  for (int r = wave; r < BM; r += 4) {
    const int m = m0 + r;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (m < n) v = *reinterpret_cast<const f32x4*>(z + (int64_t)m * D + lane * 4);
    float s = 0.f;
#pragma unroll
    for (int e = 0; e < 4; ++e) s = fmaf(v[e], v[e], s);
    s = wave_sum(s);
    if (lane == 0) zz_s[r] = s;
  }

  // ---- staging: loads are unconditional from clamped addresses, validity is applied at the LDS store
  const int col4 = tid % KQ, row0 = tid / KQ;
  const float* a_src[A_F4];
  unsigned a_ok = 0u;
#pragma unroll
  for (int i = 0; i < A_F4; ++i) {
    const int m = m0 + row0 + RPP * i;
    const bool ok = m < n;
    a_src[i] = z + (int64_t)(ok ? m : 0) * D + col4 * 4;
    if (ok) a_ok |= 1u << i;
  }
  f32x4 ra[A_F4], rb[B_F4];
  float ss[B_F4];  // running sum e^2 of this thread's 4 columns of code row (row0 + RPP i), over the K tiles
#pragma unroll
  for (int i = 0; i < B_F4; ++i) ss[i] = 0.f;

  auto load_a = [&](int i, int g) { ra[i] = *reinterpret_cast<const f32x4*>(a_src[i] + (g % NKT) * BK); };
  auto load_b = [&](int i, int g) {
    const int code = (g / NKT) * BN + row0 + RPP * i;
    rb[i] = *reinterpret_cast<const f32x4*>(Bg + (int64_t)(code < n_e ? code : 0) * D + (g % NKT) * BK + col4 * 4);
  };
  auto store_a = [&](int i, int buf) {
    f32x4 v = ra[i];
    const bool ok = (a_ok >> i) & 1u;
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = ok ? v[e] : 0.f;
    *reinterpret_cast<f32x4*>(As + buf * BM * LDS_LD + (row0 + RPP * i) * LDS_LD + col4 * 4) = v;
  };
  // tile g's piece i of the code operand; with the last K tile of a code tile the code norms are complete
  auto store_b = [&](int i, int g, int buf) {
    f32x4 v = rb[i];
    const bool ok = (g / NKT) * BN + row0 + RPP * i < n_e;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      v[e] = ok ? v[e] : 0.f;
      ss[i] = fmaf(v[e], v[e], ss[i]);
    }
    *reinterpret_cast<f32x4*>(Bs + buf * BN * LDS_LD + (row0 + RPP * i) * LDS_LD + col4 * 4) = v;
    if (g % NKT == NKT - 1) {  // (uniform)
      float s = ss[i];
      s += __shfl_xor(s, 1, 64);
      s += __shfl_xor(s, 2, 64);
      s += __shfl_xor(s, 4, 64);
      if (col4 == 0) ee_s[(g / NKT) & 1][row0 + RPP * i] = s;
      ss[i] = 0.f;
    }
  };

  // ---- prologue: tile 0 -> LDS[0]; tile 1 -> registers
#pragma unroll
  for (int i = 0; i < B_F4; ++i) load_b(i, 0);
#pragma unroll
  for (int i = 0; i < A_F4; ++i) load_a(i, 0);
#pragma unroll
  for (int i = 0; i < B_F4; ++i) store_b(i, 0, 0);
#pragma unroll
  for (int i = 0; i < A_F4; ++i) store_a(i, 0);
#pragma unroll
  for (int i = 0; i < B_F4; ++i) load_b(i, 1);  // (G >= NKT = 8: tile 1 exists)
#pragma unroll
  for (int i = 0; i < A_F4; ++i) load_a(i, 1);
  __syncthreads();

  float zz[16], best[16];
  int best_j[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    zz[r] = zz_s[wm0 + (r & 3) + 8 * (r >> 2) + 4 * hh];
    best[r] = INFINITY;
    best_j[r] = -1;
  }
  f32x16 acc[TN];
#pragma unroll
  for (int tj = 0; tj < TN; ++tj)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[tj][r] = 0.f;

  // ---- main loop.  While tile g is multiplied out of LDS[g & 1], the registers (tile g + 1) are written to the
  // other buffer and refilled with tile g + 2, one float4 piece after each of the last MFMA steps.
  for (int g = 0; g < G; ++g) {
    const int buf = g & 1;
    const bool has_next = g + 1 < G;        // (uniform) the registers hold a real tile
    const int g2 = g + 2 < G ? g + 2 : G - 1;  // clamped: a harmless duplicate load at the tail
    const float* Ab = As + buf * BM * LDS_LD + (wm0 + l31) * LDS_LD + (BK / 2) * hh;
    const float* Bb = Bs + buf * BN * LDS_LD + (wn0 + l31) * LDS_LD + (BK / 2) * hh;
    f32x4 af[2], bf[2][TN];
    af[0] = *reinterpret_cast<const f32x4*>(Ab);
#pragma unroll
    for (int tj = 0; tj < TN; ++tj) bf[0][tj] = *reinterpret_cast<const f32x4*>(Bb + tj * 32 * LDS_LD);
#pragma unroll
    for (int j = 0; j < BK / 8; ++j) {
      if (j + 1 < BK / 8) {  // next group's fragments fly under this group's MFMAs
        af[(j + 1) & 1] = *reinterpret_cast<const f32x4*>(Ab + 4 * (j + 1));
#pragma unroll
        for (int tj = 0; tj < TN; ++tj)
          bf[(j + 1) & 1][tj] = *reinterpret_cast<const f32x4*>(Bb + tj * 32 * LDS_LD + 4 * (j + 1));
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) {
#pragma unroll
        for (int tj = 0; tj < TN; ++tj)
          acc[tj] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[j & 1][e], bf[j & 1][tj][e], acc[tj], 0, 0, 0);
        const int s = 4 * j + e;
        // staging pieces pinned after MFMA step s: B pieces first, each stored and at once re-loaded
#pragma unroll
        for (int q = 0; q < 2 * NPIECE; ++q) {
          if (FIRST + q != s) continue;
          __builtin_amdgcn_sched_barrier(0);
          const int pc = q >> 1;
          if ((q & 1) == 0) {
            if (has_next) {
              if (pc < B_F4) store_b(pc, g + 1, buf ^ 1);
              else store_a(pc - B_F4, buf ^ 1);
            }
          } else {
            if (pc < B_F4) load_b(pc, g2);
            else load_a(pc - B_F4, g2);
          }
          __builtin_amdgcn_sched_barrier(0);
        }
      }
    }
    if (g % NKT == NKT - 1) {  // (uniform) a code tile is complete: fold it into the running minima
      const int ct = g / NKT;
#pragma unroll
      for (int tj = 0; tj < TN; ++tj) {
        const int cl = wn0 + tj * 32 + l31;
        const int code = ct * BN + cl;
        const float ee = ee_s[ct & 1][cl];
        const bool valid = code < n_e;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float d = (zz[r] + ee) - 2.0f * acc[tj][r];
          if (valid && d < best[r]) {
            best[r] = d;
            best_j[r] = code;
          }
          acc[tj][r] = 0.f;
        }
      }
    }
    __syncthreads();
  }

  // ---- combine: the 32 lanes that hold a row's codes, then the WARPS_N waves of the row
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    float b = best[r];
    int bj = best_j[r];
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) {
      const float ob = __shfl_xor(b, o, 64);
      const int oj = __shfl_xor(bj, o, 64);
      fit_take(b, bj, ob, oj);
    }
    if (l31 == 0) {
      const int rl = wm0 + (r & 3) + 8 * (r >> 2) + 4 * hh;
      red_v[wn][rl] = b;
      red_j[wn][rl] = bj;
    }
  }
  __syncthreads();
  if (tid < BM && m0 + tid < n) {
    float b = red_v[0][tid];
    int bj = red_j[0][tid];
#pragma unroll
    for (int w = 1; w < WARPS_N; ++w) fit_take(b, bj, red_v[w][tid], red_j[w][tid]);
    const int64_t o = (int64_t)(m0 + tid) * n_books + book;
    dmin[o] = b;
    if (jmin) jmin[o] = bj;
  }
}

// One workgroup per (image, group); thread h sums its book's column over the group's rows in ascending row order
// (float64, fixed order: reproducible and independent of the batch), thread 0 decides.
__global__ __launch_bounds__(64) void texture_vote_kernel(const float* __restrict__ dmin,
                                                          const int64_t* __restrict__ segm_tok, int T, int n_books,
                                                          double* __restrict__ cost, int32_t* __restrict__ count,
                                                          int64_t* __restrict__ attr) {
  __shared__ double cs[64];
  const int b = blockIdx.x / 3, grp = blockIdx.x % 3;
  const int h = threadIdx.x;
  const int64_t* lab = segm_tok + (int64_t)b * T;
  const float* dm = dmin + (int64_t)b * T * n_books;
  double c = 0.0;
  int cnt = 0;
  for (int t = 0; t < T; ++t) {
    const int64_t l = lab[t];
    const bool in = grp == 0 ? (l == 1 || l == 4) : grp == 1 ? (l == 3 || l == 5 || l == 21) : (l == 2);
    if (!in) continue;  // (uniform: every thread reads the same label)
    ++cnt;
    if (h < n_books) c += (double)dm[(int64_t)t * n_books + h];
  }
  if (h < n_books) {
    cs[h] = c;
    cost[((int64_t)b * 3 + grp) * n_books + h] = c;
  }
  __syncthreads();
  if (h == 0) {
    count[b * 3 + grp] = cnt;
    double bestc = INFINITY;
    int bh = -1;
    if (cnt > 0)
      for (int k = 0; k < n_books; ++k)
        if (cs[k] < bestc) {  // first least cost; +inf / NaN never chosen
          bestc = cs[k];
          bh = k;
        }
    attr[b * 3 + grp] = bh <= 0 ? 17 : bh - 1;  // inverse of the mask rule: value 0 = no texture = attribute 17
  }
}

thread_local int g_fit_force_bm = 0;  // tests / measurements of the calling thread: t2h_vq_fit_force_tile()

}  // namespace

extern "C" int t2h_vq_fit_force_tile(int bm) {
  const int old = g_fit_force_bm;
  g_fit_force_bm = (bm == 32 || bm == 64 || bm == 128) ? bm : 0;
  return old;
}

extern "C" int t2h_vq_fit_books_f32(const float* z, const float* books, float* dmin, int32_t* jmin, int32_t n,
                                    int32_t n_books, int32_t n_e, int32_t d, void* stream) {
  T2H_REQUIRE(z && books && dmin, "t2h_vq_fit_books_f32: NULL pointer");
  T2H_REQUIRE(n > 0 && n_books > 0 && n_e > 0, "t2h_vq_fit_books_f32: empty problem n=%d n_books=%d n_e=%d", n, n_books, n_e);
  if (d != FIT_D) {
    t2h_set_error("t2h_vq_fit_books_f32: d=%d unsupported (256)", d);
    return T2H_ERR_UNSUPPORTED;
  }
  T2H_REQUIRE(t2h_aligned16(z) && t2h_aligned16(books), "t2h_vq_fit_books_f32: 16-byte alignment");
  T2H_REQUIRE((int64_t)n * n_books < (1ll << 31) && (int64_t)((n + 31) / 32) * n_books < (1ll << 31),
              "t2h_vq_fit_books_f32: n=%d x n_books=%d too large", n, n_books);
  hipStream_t s = static_cast<hipStream_t>(stream);
  // Row tile: the largest that still gives every CU (256) a workgroup.  The choice changes no bit of the result.
  int bm = g_fit_force_bm;
  if (bm == 0) bm = (int64_t)((n + 127) / 128) * n_books >= 256 ? 128 : (int64_t)((n + 63) / 64) * n_books >= 256 ? 64 : 32;
  const dim3 grid((unsigned)(((n + bm - 1) / bm) * n_books)), block(FIT_NT);
  if (bm == 128) hipLaunchKernelGGL((vq_fit_kernel<4, 1>), grid, block, 0, s, z, books, dmin, jmin, n, n_books, n_e);
  else if (bm == 64) hipLaunchKernelGGL((vq_fit_kernel<2, 2>), grid, block, 0, s, z, books, dmin, jmin, n, n_books, n_e);
  else hipLaunchKernelGGL((vq_fit_kernel<1, 4>), grid, block, 0, s, z, books, dmin, jmin, n, n_books, n_e);
  T2H_CHECK_LAUNCH("t2h_vq_fit_books_f32");
  return T2H_OK;
}

extern "C" int t2h_texture_vote(const float* dmin, const int64_t* segm_tok, int32_t B, int32_t T, int32_t n_books,
                                double* cost, int32_t* count, int64_t* attr, void* stream) {
  T2H_REQUIRE(dmin && segm_tok && cost && count && attr, "t2h_texture_vote: NULL pointer");
  T2H_REQUIRE(B > 0 && T > 0 && n_books > 0 && n_books <= 64, "t2h_texture_vote: bad shape B=%d T=%d n_books=%d (<= 64)", B, T,
              n_books);
  hipLaunchKernelGGL(texture_vote_kernel, dim3(3 * B), dim3(64), 0, static_cast<hipStream_t>(stream), dmin, segm_tok, T,
                     n_books, cost, count, attr);
  T2H_CHECK_LAUNCH("t2h_texture_vote");
  return T2H_OK;
}
