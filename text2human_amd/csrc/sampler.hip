// Index-sampler glue kernels: 4-way embedding sum, the unmasking schedule step
// and the texture-routed categorical sampling tail.
#include "common.h"

namespace {

// x[row] = ((tok_emb[idx] + pos_emb[t]) + segm_emb[segm]) + texture_emb[tex]
// -- same association order as models/archs/transformer_arch.py:266.
__global__ void embed_sum4_kernel(const int64_t* __restrict__ idx, const int64_t* __restrict__ segm,
                                  const int64_t* __restrict__ tex, const float* __restrict__ tok_emb,
                                  const float* __restrict__ pos_emb, const float* __restrict__ segm_emb,
                                  const float* __restrict__ tex_emb, float* __restrict__ x, int T,
                                  int C) {
  const int row = blockIdx.x;
  const int t = row % T;
  const float* a = tok_emb + idx[row] * C;
  const float* b = pos_emb + (int64_t)t * C;
  const float* c = segm_emb + segm[row] * C;
  const float* d = tex_emb + tex[row] * C;
  float* o = x + (int64_t)row * C;
  for (int i = threadIdx.x * 4; i < C; i += blockDim.x * 4) {
    const f32x4 va = *reinterpret_cast<const f32x4*>(a + i);
    const f32x4 vb = *reinterpret_cast<const f32x4*>(b + i);
    const f32x4 vc = *reinterpret_cast<const f32x4*>(c + i);
    const f32x4 vd = *reinterpret_cast<const f32x4*>(d + i);
    *reinterpret_cast<f32x4*>(o + i) = ((va + vb) + vc) + vd;
  }
}

// changes = rand < 1/t ; changes &= ~unmasked ; unmasked |= changes
// (models/sample_model.py:286-292).  `1 / t.float()` is an fp32 reciprocal.
// With changed_rows: the changed tokens are also appended to that list (in no particular
// order -- every row is sampled independently) and counted in head_count[n_heads].
__global__ void unmask_step_kernel(const float* __restrict__ rnd, float thresh,
                                   uint8_t* __restrict__ unmasked, uint8_t* __restrict__ changes,
                                   const int64_t* __restrict__ tex, int* __restrict__ head_count,
                                   int n, int* __restrict__ changed_rows, int n_heads) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const bool um = unmasked[i] != 0;
  const bool ch = (rnd[i] < thresh) && !um;
  changes[i] = ch ? 1 : 0;
  if (ch) {
    unmasked[i] = 1;
    atomicAdd(head_count + (int)tex[i], 1);
    if (changed_rows) changed_rows[atomicAdd(head_count + n_heads, 1)] = i;
  }
}

// ---- truncated sampling (top-k / top-p; DESIGN.md, "Truncated sampling").  Truncation is ONE threshold per row: class j
// enters the race iff l_j >= theta.  theta comes from a most-significant-digit radix select over order-preserving
// 32-bit keys of the row's temperature-scaled logits, 8 bits per pass: a count histogram (top-k: the smallest value
// with fewer than k values above it) and a 64-bit INTEGER mass histogram (top-p: m_j = floor(expf(l_j - max) 2^32),
// the smallest surviving value v with G(v) 2^20 < p_q S, G(v) = mass strictly above v, S = mass of the top-k
// survivors).  Only integers are accumulated, so the kept set does not depend on the order of the LDS atomics nor on
// how the values are spread over threads: the workgroup form (NT = 1024) and the wave form (NT = 64) are this one
// function.
constexpr int TR_BINS = 256;
struct trunc_lds {
  uint32_t cnt[TR_BINS];
  unsigned long long mass[TR_BINS];
  unsigned long long sel_mass;                // mass above the selected bin
  uint32_t sel_digit, sel_above, sel_in_bin;  // the selected bin, the values above it, the values in it
};
__device__ __forceinline__ uint32_t trunc_key(float l) {  // a < b <=> key(a) < key(b); -0 and +0 are one value
  uint32_t u = __builtin_bit_cast(uint32_t, l);
  if (l == 0.f) u = 0;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float trunc_unkey(uint32_t k) {
  return __builtin_bit_cast(float, (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}
__device__ __forceinline__ unsigned long long trunc_mass(float l, float mx) {
  float e = expf(l - mx);  // the value the race evaluates, in [0, 1]
  e = e >= 0.f ? e : 0.f;  // (NaN rows: no mass)
  return (unsigned long long)((double)e * 4294967296.0);  // exact scaling, then floor
}
template <int NT>
__device__ __forceinline__ void trunc_sync() {
  if (NT == 64) {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // one wave: its own LDS traffic has landed
  } else {
    __syncthreads();
  }
}
// -> key of theta (0: nothing is cut), *kept = number of surviving classes.  All NT threads call it; t = 0 .. NT - 1;
// thread t owns lg[t], lg[t + NT], ...; top_k == 0 / p_q == 0: that rule is off (not both).
template <int NT>
__device__ __forceinline__ uint32_t trunc_select(const float* lg, int n_class, float mx, int top_k, uint32_t p_q,
                                                 trunc_lds* L, int t, int* kept) {
  for (int b = t; b < TR_BINS; b += NT) {
    L->cnt[b] = 0;
    L->mass[b] = 0;
  }
  trunc_sync<NT>();
  uint32_t floor_key = 0;  // survivors so far: key >= floor_key
  int n_kept = n_class;
  for (int stage = 0; stage < 2; ++stage) {
    const bool by_mass = stage == 1;
    if (by_mass ? p_q == 0 : top_k == 0) continue;
    uint32_t prefix = 0, above_c = 0, in_bin = 0;
    unsigned long long above_m = 0, S = 0;
    for (int shift = 24; shift >= 0; shift -= 8) {
      for (int j = t; j < n_class; j += NT) {
        const float l = lg[j];
        const uint32_t key = trunc_key(l);
        if (key < floor_key || (shift < 24 && (key >> (shift + 8)) != prefix)) continue;
        const int d = (key >> shift) & (TR_BINS - 1);
        __hip_atomic_fetch_add(&L->cnt[d], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (by_mass) __hip_atomic_fetch_add(&L->mass[d], trunc_mass(l, mx), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      }
      trunc_sync<NT>();
      if (t < 64) {  // the first wave: 4 bins per lane, sums of the bins above by a butterfly; leaves the bins zeroed
        uint32_t c[4], tot_c = 0, suf_c = 0;
        unsigned long long m[4], tot_m = 0, suf_m = 0;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          c[b] = L->cnt[4 * t + b];
          m[b] = L->mass[4 * t + b];
          L->cnt[4 * t + b] = 0;
          L->mass[4 * t + b] = 0;
          tot_c += c[b];
          tot_m += m[b];
        }
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
          const uint32_t oc = __shfl_xor(tot_c, o, 64);
          const unsigned long long om = __shfl_xor(tot_m, o, 64);
          if (!(t & o)) {
            suf_c += oc;
            suf_m += om;
          }
          tot_c += oc;
          tot_m += om;
        }
        if (shift == 24) S = tot_m;  // the first pass of a stage sees every survivor
        // the smallest non-empty bin whose largest value still qualifies (the predicate is monotone in the value)
        int cand = TR_BINS;
        uint32_t ac = above_c + suf_c, cand_c = 0, cand_n = 0;
        unsigned long long am = above_m + suf_m, cand_m = 0;
#pragma unroll
        for (int b = 3; b >= 0; --b) {
          const bool ok = by_mass ? (am << 20) < (unsigned long long)p_q * S : ac < (uint32_t)top_k;
          if (c[b] > 0 && ok) {
            cand = 4 * t + b;
            cand_c = ac;
            cand_m = am;
            cand_n = c[b];
          }
          ac += c[b];
          am += m[b];
        }
        int first = cand;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) first = min(first, __shfl_xor(first, o, 64));
        if (first == TR_BINS) {  // (only rows of NaNs / infinities without any mass: nothing to select, no fault)
          first = TR_BINS - 1;
          cand = t == 0 ? first : TR_BINS;
          cand_c = above_c;
          cand_m = above_m;
          cand_n = 0;
        }
        if (cand == first) {
          L->sel_digit = (uint32_t)first;
          L->sel_above = cand_c;
          L->sel_mass = cand_m;
          L->sel_in_bin = cand_n;
        }
      }
      trunc_sync<NT>();
      prefix = (prefix << 8) | L->sel_digit;
      above_c = L->sel_above;
      above_m = L->sel_mass;
      in_bin = L->sel_in_bin;
    }
    floor_key = prefix;
    n_kept = (int)(above_c + in_bin);
  }
  *kept = n_kept;
  return floor_key;
}

// ---- per-image sampling controls ("Per-image sampling controls").  The PER_SAMPLE instances of the tail
// kernels take temp / top_k / top_p_q of row `row` from params[row / T] (T = rows per sample, the batch in its device
// order) instead of the launch's scalars; everything else is the scalar instance's code.  The table lives in device
// memory, so the values are normalised here the way trunc_settings normalises the scalars on the host: an image whose
// rules cut nothing has (0, 0) and skips the selection (theta = -inf: every class enters the race).
struct sample_settings {
  float temp;
  int top_k;
  uint32_t top_p_q;
};
template <bool PER_SAMPLE>
__device__ __forceinline__ sample_settings row_settings(float temp, int top_k, uint32_t top_p_q,
                                                       const t2h_sample_params* __restrict__ params, int row, int T,
                                                       int n_class) {
  sample_settings s = {temp, top_k, top_p_q};
  if constexpr (PER_SAMPLE) {
    const t2h_sample_params p = params[row / T];  // (row is uniform over the wave: one scalar load)
    s.temp = p.temp;
    s.top_k = (p.top_k <= 0 || p.top_k >= n_class) ? 0 : p.top_k;
    s.top_p_q = p.top_p_q >= (1u << 20) ? 0u : p.top_p_q;
  }
  return s;
}

// ---- the pieces of the sampling tail, each written once: LN_f of a row, the head's dot products, the row maximum, the
// truncation threshold and the exponential race.  Every tail kernel below is made of these, so two kernels that form
// the same quantity form the same bits.
constexpr int SH_THREADS = 1024;  // one workgroup per token row
constexpr int CP_ROWS = 4;        // the wave form: one wave per token row, CP_ROWS rows per workgroup

// One wave, one C-wide row: lane l holds floats 4 l .. 4 l + 3 of every 256.
template <int VPL>
__device__ __forceinline__ void load_row(const float* p, int lane, f32x4 (&w)[VPL]) {
#pragma unroll
  for (int i = 0; i < VPL; ++i) w[i] = *reinterpret_cast<const f32x4*>(p + i * 256 + lane * 4);
}
// v = LN_f(xr), eps = 1e-5
template <int C>
__device__ __forceinline__ void lnf_row(const float* xr, const float* __restrict__ g, const float* __restrict__ bta,
                                        int lane, f32x4 (&v)[C / 256]) {
  constexpr int VPL = C / 256;
  load_row(xr, lane, v);
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < VPL; ++i) s += (v[i][0] + v[i][1]) + (v[i][2] + v[i][3]);
  const float mean = wave_sum(s) * (1.0f / C);
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < VPL; ++i)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float d = v[i][e] - mean;
      q = fmaf(d, d, q);
    }
  const float rstd = 1.0f / sqrtf(wave_sum(q) * (1.0f / C) + 1e-5f);
  f32x4 gg[VPL], bb[VPL];
  load_row(g, lane, gg);
  load_row(bta, lane, bb);
#pragma unroll
  for (int i = 0; i < VPL; ++i)
#pragma unroll
    for (int e = 0; e < 4; ++e) v[i][e] = (v[i][e] - mean) * rstd * gg[i][e] + bb[i][e];
}
// This lane's share of <w, v>: one fma chain in element order (wave_sum of it is the logit)
template <int VPL>
__device__ __forceinline__ float lane_dot(const f32x4 (&w)[VPL], const f32x4 (&v)[VPL]) {
  float t = 0.f;
#pragma unroll
  for (int i = 0; i < VPL; ++i)
#pragma unroll
    for (int e = 0; e < 4; ++e) t = fmaf(w[i][e], v[i][e], t);
  return t;
}
// acc[u] = this lane's share of <w[j0 + u], v>, u = 0 .. 3 (classes past the end repeat the last one): a wave takes 4
// classes per iteration so that 8 independent 1-KiB weight-row loads are in flight (the loop is latency bound).  The
// caller finishes each with wave_sum next to its guarded store.
template <int C>
__device__ __forceinline__ void head_dot4(const float* __restrict__ w, int j0, int n_class, int lane,
                                          const f32x4 (&v)[C / 256], float (&acc)[4]) {
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    f32x4 ww[C / 256];
    load_row(w + (int64_t)min(j0 + u, n_class - 1) * C, lane, ww);
    acc[u] = lane_dot(ww, v);
  }
}

// Maximum over the NT threads of a row: a wave (NT == 64), or a workgroup through red[NT / 64].  The workgroup form
// holds ONE barrier, after which everything the threads wrote to LDS before the call is visible as well.
template <int NT>
__device__ __forceinline__ float block_max(float mx, float* red, int lane, int wave) {
  mx = wave_max(mx);
  if constexpr (NT != 64) {
    if (lane == 0) red[wave] = mx;
    __syncthreads();
    mx = red[0];
#pragma unroll
    for (int k = 1; k < NT / 64; ++k) mx = fmaxf(mx, red[k]);
  }
  return mx;
}
// thread t = 0 .. NT - 1 of the row owns lg[t], lg[t + NT], ...
template <int NT>
__device__ __forceinline__ float row_max(const float* lg, int n_class, int t, float* red, int lane, int wave) {
  float mx = -INFINITY;
  for (int j = t; j < n_class; j += NT) mx = fmaxf(mx, lg[j]);
  return block_max<NT>(mx, red, lane, wave);
}

// se = sum_j expf(lg[j] - mx) over ALL classes of the row, in an order that is part of the definition: thread t adds its
// classes t, t + NT, ... in ascending order, wave_sum, and (NT != 64) the waves' sums are added in wave order through
// reds[NT / 64].  Every thread returns the sum.  The workgroup form holds one barrier before its LDS writes (whoever
// read reds[] before the call has finished) and one after them.  log p(tok) = (lg[tok] - mx) - logf(se).
template <int NT>
__device__ __forceinline__ float row_logsum(const float* lg, int n_class, float mx, int t, float* reds, int lane, int wave) {
  float se = 0.f;
  for (int j = t; j < n_class; j += NT) se += expf(lg[j] - mx);
  se = wave_sum(se);
  if constexpr (NT != 64) {
    __syncthreads();
    if (lane == 0) reds[wave] = se;
    __syncthreads();
    se = reds[0];
#pragma unroll
    for (int k = 1; k < NT / 64; ++k) se += reds[k];
  }
  return se;
}

// theta of the row (class j enters the race iff lg[j] >= theta); -inf where nothing is cut.  The selection's LDS is one
// object per workgroup, or one per wave in the wave form.
template <int NT, bool TRUNC, bool PER_SAMPLE>
__device__ __forceinline__ float row_theta(const float* lg, int n_class, float mx, int top_k, uint32_t top_p_q, int t) {
  float theta = -INFINITY;
  if constexpr (TRUNC) {
    __shared__ trunc_lds tr[NT == 64 ? CP_ROWS : 1];
    int kept;
    if (!PER_SAMPLE || top_k != 0 || top_p_q != 0)  // (uniform over the wave / workgroup)
      theta = trunc_unkey(trunc_select<NT>(lg, n_class, mx, top_k, top_p_q, &tr[NT == 64 ? threadIdx.x >> 6 : 0], t, &kept));
  }
  return theta;
}

// The exponential race: argmax_j exp(l_j - max) / q_j, the first index wins ties.
struct race {
  float best = -1.f;
  int j = 0x7fffffff;
  __device__ __forceinline__ void offer(float sc, int jj) {  // (a thread offers its classes in ascending order)
    if (sc > best) {
      best = sc;
      j = jj;
    }
  }
  __device__ __forceinline__ void wave_reduce() {  // every lane ends with the wave's winner
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ob = __shfl_xor(best, o, 64);
      const int oj = __shfl_xor(j, o, 64);
      if (ob > best || (ob == best && oj < j)) {
        best = ob;
        j = oj;
      }
    }
  }
  // after wave_reduce: the workgroup's winner, on thread 0 only.  red[] / redj[]: NW slots each; red[] may be the
  // array block_max used (the first barrier: every thread has read it).
  template <int NW>
  __device__ __forceinline__ void block_reduce(float* red, int* redj, int tid) {
    __syncthreads();
    if ((tid & 63) == 0) {
      red[tid >> 6] = best;
      redj[tid >> 6] = j;
    }
    __syncthreads();
    if (tid == 0)
      for (int k = 1; k < NW; ++k)
        if (red[k] > best || (red[k] == best && redj[k] < j)) {
          best = red[k];
          j = redj[k];
        }
  }
  // all-NaN scores (only after a flagged split-precision overflow upstream): keep the token id
  // inside the embedding table so the run reaches the host-side overflow check instead of faulting
  __device__ __forceinline__ int winner(int n_class) const { return j >= n_class ? 0 : j; }
};

// One workgroup per token row; rows that are not (changed && of this head's
// texture) exit at once.  LN_f -> 512->n_class head (wave-cooperative dot
// products, coalesced weight rows) -> exponential-race argmax.
template <int C, bool TRUNC = false, bool PER_SAMPLE = false, bool LOGP = false>
__device__ __forceinline__ void sample_row(float* lds, int row, const float* __restrict__ hidden,
                                           const float* __restrict__ g, const float* __restrict__ bta,
                                           const float* __restrict__ w, const float* __restrict__ expo, int head,
                                           float temp, int64_t* __restrict__ x_t,
                                           int64_t* __restrict__ out_idx, int n_class, int top_k = 0,
                                           uint32_t top_p_q = 0, float* __restrict__ logp = nullptr) {
  constexpr int NW = SH_THREADS / 64;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  f32x4 v[C / 256];
  lnf_row<C>(hidden + (int64_t)row * C, g, bta, lane, v);
  for (int j0 = wave * 4; j0 < n_class; j0 += NW * 4) {
    float acc[4];
    head_dot4<C>(w, j0, n_class, lane, v, acc);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const float r = wave_sum(acc[u]);
      if (lane == 0 && j0 + u < n_class) lds[j0 + u] = r / temp;  // (the reference divides: logits / temp, sample_model.py:303)
    }
  }
  __syncthreads();
  float* red = lds + n_class;
  const float mx = row_max<SH_THREADS>(lds, n_class, tid, red, lane, wave);
  const float theta = row_theta<SH_THREADS, TRUNC, PER_SAMPLE>(lds, n_class, mx, top_k, top_p_q, tid);
  const float* er = expo + (int64_t)row * n_class;
  race best;
  for (int j = tid; j < n_class; j += SH_THREADS) {
    if (TRUNC && !(lds[j] >= theta)) continue;
    best.offer(expf(lds[j] - mx) / er[j], j);
  }
  best.wave_reduce();
  best.block_reduce<NW>(red, reinterpret_cast<int*>(red + NW), tid);
  if (tid == 0) {
    x_t[row] = (int64_t)best.winner(n_class) + (int64_t)n_class * head;
    out_idx[row] = best.winner(n_class);
  }
  if constexpr (LOGP) {  // (after the race: its barrier frees red[] once thread 0 has read the winner)
    const float se = row_logsum<SH_THREADS>(lds, n_class, mx, tid, red, lane, wave);
    if (tid == 0) logp[row] = (lds[best.winner(n_class)] - mx) - logf(se);
  }
}

template <int C>
__global__ __launch_bounds__(SH_THREADS) void sample_head_kernel(
    const float* __restrict__ hidden, const float* __restrict__ g, const float* __restrict__ bta,
    const float* __restrict__ w, const float* __restrict__ expo, const uint8_t* __restrict__ changes,
    const int64_t* __restrict__ tex, int head, float temp, int64_t* __restrict__ x_t,
    int64_t* __restrict__ out_idx, int n_class) {
  extern __shared__ __attribute__((aligned(16))) float lds[];  // n_class logits + 2*NW reduce slots
  const int row = blockIdx.x;
  if (!changes[row] || (int)tex[row] != head) return;
  sample_row<C>(lds, row, hidden, g, bta, w, expo, head, temp, x_t, out_idx, n_class);
}

// ---- sampler training-time forward (models/transformer_model.py:212-274, forward only)
// q_sample: mask = u < t/T (fp32 division, like t.float() / num_timesteps); x_t = mask ? mask_id : x_0
__global__ void q_sample_kernel(const int64_t* __restrict__ x0, const float* __restrict__ u,
                                const int64_t* __restrict__ t, float num_timesteps, int64_t mask_id,
                                int64_t* __restrict__ x_t, uint8_t* __restrict__ mask, int T, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const bool m = u[i] < (float)t[i / T] / num_timesteps;
  mask[i] = m ? 1 : 0;
  x_t[i] = m ? mask_id : x0[i];
}

// Cross entropy of the masked tokens.  F.cross_entropy(..., ignore_index=-1) summed over the
// 18 heads only ever sees the head of the token's own texture (every other head's target is
// -1), so: one workgroup per token, rows that are unmasked or have target -1 contribute 0,
// the others LN_f -> head of their texture -> logsumexp(logits) - logits[target].
template <int C>
__global__ __launch_bounds__(SH_THREADS) void masked_ce_kernel(
    const float* __restrict__ hidden, const float* __restrict__ g, const float* __restrict__ bta,
    const float* __restrict__ w_heads, const int64_t* __restrict__ tex, const uint8_t* __restrict__ mask,
    const int64_t* __restrict__ gt_lists, float* __restrict__ ce, int n, int n_class, int n_heads) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int row = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int head = (int)tex[row];
  const int64_t target = (head >= 0 && head < n_heads) ? gt_lists[(int64_t)head * n + row] : -1;
  if (!mask[row] || target < 0) {
    if (tid == 0) ce[row] = 0.f;
    return;
  }
  f32x4 v[C / 256];
  lnf_row<C>(hidden + (int64_t)row * C, g, bta, lane, v);
  constexpr int NW = SH_THREADS / 64;
  const float* w = w_heads + (int64_t)head * n_class * C;
  for (int j = wave; j < n_class; j += NW) {
    f32x4 ww[C / 256];
    load_row(w + (int64_t)j * C, lane, ww);
    const float a = wave_sum(lane_dot(ww, v));
    if (lane == 0) lds[j] = a;
  }
  __syncthreads();
  float* red = lds + n_class;
  const float mx = row_max<SH_THREADS>(lds, n_class, tid, red, lane, wave);
  float se = 0.f;
  for (int j = tid; j < n_class; j += SH_THREADS) se += expf(lds[j] - mx);
  se = wave_sum(se);
  __syncthreads();
  if (lane == 0) red[wave] = se;
  __syncthreads();
  if (tid == 0) {
    float tot = 0.f;
    for (int k = 0; k < NW; ++k) tot += red[k];
    ce[row] = (mx + logf(tot)) - lds[target];
  }
}

// out[b] = sum_t x[b][t] in a fixed order (one workgroup per segment)
__global__ __launch_bounds__(256) void segment_sum_kernel(const float* __restrict__ x, float* __restrict__ out,
                                                          int T) {
  __shared__ float red[4];
  const int b = blockIdx.x, tid = threadIdx.x;
  float s = 0.f;
  for (int i = tid; i < T; i += 256) s += x[(int64_t)b * T + i];
  s = wave_sum(s);
  if ((tid & 63) == 0) red[tid >> 6] = s;
  __syncthreads();
  if (tid == 0) out[b] = (red[0] + red[1]) + (red[2] + red[3]);
}

// ---- torch's `exponential_` draw, element by element.  The reference's Categorical.sample() draws
// a FULL [n, n_class] Exp(1) tensor per active head from the device Philox generator
// (models/sample_model.py:305-306 -> multinomial -> exponential_) although only the changed rows of
// that head use it.  ATen's kernel (distribution_elementwise_grid_stride_kernel, unroll 4, block 256,
// grid G) gives element e of the tensor the value
//     u = uniform( philox4x32_10(key = seed, counter = {offset/4 + it, subsequence = idx})[ii] ),
//     idx = e % (256 G), it = e / (256 G) / 4, ii = e / (256 G) % 4,
//     q = u >= 1 - 2^-24 ? 2^-24 : -log(u)
// (curand_init(seed, idx, offset) / curand_uniform4 = rocRAND's philox4x32_10 engine and
// uniform_distribution; transformation::exponential of ATen/core/TransformationHelper.h).  Computing
// it here for the (row, class) pairs that are actually used is bit-identical
// (tests/test_gpu_kernels.py: full-tensor equality with torch) and removes a 16 MB draw per active
// head and step.
__device__ __forceinline__ void philox_round(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
  const uint64_t m0 = (uint64_t)0xD2511F53u * c[0], m1 = (uint64_t)0xCD9E8D57u * c[2];
  const uint32_t hi0 = (uint32_t)(m0 >> 32), lo0 = (uint32_t)m0, hi1 = (uint32_t)(m1 >> 32), lo1 = (uint32_t)m1;
  const uint32_t n0 = hi1 ^ c[1] ^ k0, n2 = hi0 ^ c[3] ^ k1;
  c[0] = n0;
  c[1] = lo1;
  c[2] = n2;
  c[3] = lo0;
}
// log(x) exactly as it is compiled into ATen's kernel: LLVM's f32 log lowering for targets with fast FMA
// (y = v_log_f32(x); r = y c; r + fma(y, cc, fma(y, c, -r)), c + cc = ln 2 to 49 bits).  Contraction
// must stay off: fusing the last add into fma(c, y, t) counts the rounding error of r twice and is off
// by one ulp for a third of the arguments (ocml's logf of ROCm 7.2 differs from ATen's build the same way).
__device__ __forceinline__ float aten_logf(float x) {
#pragma clang fp contract(off)
  const float y = __builtin_amdgcn_logf(x), c = 0x1.62e42ep-1f, cc = 0x1.efa39ep-25f;
  const float r = y * c;
  const float t = __builtin_fmaf(y, cc, __builtin_fmaf(y, c, -r));
  return r + t;
}
// word of element e of a whole-tensor draw, and curand_uniform's (0, 1] value of a word
__device__ __forceinline__ uint32_t torch_philox_word(uint64_t seed, uint64_t offset, uint32_t grid_threads, uint64_t e) {
  const uint64_t idx = e % grid_threads, m = e / grid_threads;
  const uint64_t ctr = offset / 4 + (m >> 2);
  uint32_t c[4] = {(uint32_t)ctr, (uint32_t)(ctr >> 32), (uint32_t)idx, (uint32_t)(idx >> 32)};
  uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    philox_round(c, k0, k1);
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return c[m & 3];
}
__device__ __forceinline__ float philox_unit(uint32_t v) {
  return __builtin_fmaf((float)v, 2.3283064365386963e-10f, 2.3283064365386963e-10f);  // (0, 1]
}
__device__ __forceinline__ float torch_exponential_at(uint64_t seed, uint64_t offset, uint32_t grid_threads, uint64_t e) {
  const float u = philox_unit(torch_philox_word(seed, offset, grid_threads, e));
  const float lg = u >= 1.0f - 5.9604644775390625e-8f ? -5.9604644775390625e-8f : aten_logf(u);
  return -lg;
}

__global__ void philox_exponential_kernel(uint64_t seed, uint64_t offset, uint32_t grid_threads, float* __restrict__ out,
                                          int64_t numel) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e < numel) out[e] = torch_exponential_at(seed, offset, grid_threads, (uint64_t)e);
}

// ---- torch's `rand` draw, element by element: the same engine / element <-> (thread, counter)
// mapping as above (distribution_elementwise_grid_stride_kernel, unroll 4) with ATen's uniform
// transform (uniform_kernel of ATen/native/cuda/DistributionTemplates.h, from = 0, to = 1):
// value = u * 1 + 0 with u = curand_uniform in (0, 1], and the bounds reversed: value == 1 -> 0.
__device__ __forceinline__ float torch_uniform_at(uint64_t seed, uint64_t offset, uint32_t grid_threads, uint64_t e) {
  const float u = philox_unit(torch_philox_word(seed, offset, grid_threads, e));
  return u == 1.0f ? 0.0f : u;
}

__global__ void philox_uniform_kernel(uint64_t seed, uint64_t offset, uint32_t grid_threads, float* __restrict__ out,
                                      int64_t numel) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e < numel) out[e] = torch_uniform_at(seed, offset, grid_threads, (uint64_t)e);
}

// ---- the WHOLE unmasking schedule of a sampling run in one launch.  Which token is unmasked at
// which step (models/sample_model.py:286-292) depends on the `rand` draws and on nothing the
// transformer computes; the generator offset of every draw depends on the schedule only through
// the number of heads that sample at a step (one full exponential_ draw per ACTIVE head, :301-306).
// So the `rand` draws are reproduced here, step after step, each at the offset the reference's
// generator would hold: off(t-1) = off(t) + rand_inc + popcount(active heads at t) * expo_inc.
// One workgroup (the steps are sequential and a step is n / 1024 Philox blocks per thread);
// outputs: step_of_row[i] = the step at which token row i changes (every row changes exactly once:
// at t = 1 the threshold is 1), head_mask[t] = bit h set iff head h samples at step t.
// KEEP (region editing, t2h_unmask_schedule_keep): rows with keep[i] != 0 start unmasked -- they are never drawn,
// never set a head bit and keep step_of_row = 0; the `rand` draws and the offset recurrence are unchanged.
constexpr int SCHED_THREADS = 1024, SCHED_MAX_STEPS = 4096;
// The loop, for one workgroup: the n rows of tex / keep / step_of_row and the steps + 1 words of head_mask it is handed.
template <bool KEEP>
__device__ __forceinline__ void unmask_schedule_rows(uint64_t seed, uint64_t offset, uint32_t rand_grid_threads,
                                                     uint32_t rand_inc, uint32_t expo_inc,
                                                     const int64_t* __restrict__ tex, const uint8_t* __restrict__ keep,
                                                     int n, int steps, int32_t* __restrict__ step_of_row,
                                                     uint32_t* __restrict__ head_mask) {
  __shared__ uint32_t mask_s[SCHED_MAX_STEPS + 1];  // one word per step: no reset, one barrier per step
  const int tid = threadIdx.x, lane = tid & 63;
  for (int e = tid; e < n; e += SCHED_THREADS) step_of_row[e] = 0;
  for (int t = tid; t <= steps; t += SCHED_THREADS) mask_s[t] = 0;
  __syncthreads();
  uint64_t off = offset;
  for (int t = steps; t >= 1; --t) {
    const float thresh = 1.0f / (float)t;  // `1 / t.float()`: an fp32 reciprocal
    uint32_t m = 0;
    for (int e = tid; e < n; e += SCHED_THREADS) {
      if (step_of_row[e] != 0) continue;  // already unmasked (written by this same thread)
      if (KEEP && keep[e] != 0) continue;  // kept row: unmasked from the start
      if (torch_uniform_at(seed, off, rand_grid_threads, (uint64_t)e) < thresh) {
        step_of_row[e] = t;
        m |= 1u << (int)tex[e];
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m |= __shfl_xor(m, o, 64);
    if (lane == 0 && m) atomicOr(&mask_s[t], m);
    __syncthreads();
    off += (uint64_t)rand_inc + (uint64_t)__popc(mask_s[t]) * expo_inc;
  }
  for (int t = tid; t <= steps; t += SCHED_THREADS) head_mask[t] = mask_s[t];
}
template <bool KEEP>
__global__ __launch_bounds__(SCHED_THREADS) void unmask_schedule_kernel(
    uint64_t seed, uint64_t offset, uint32_t rand_grid_threads, uint32_t rand_inc, uint32_t expo_inc,
    const int64_t* __restrict__ tex, const uint8_t* __restrict__ keep, int n, int steps,
    int32_t* __restrict__ step_of_row, uint32_t* __restrict__ head_mask) {
  unmask_schedule_rows<KEEP>(seed, offset, rand_grid_threads, rand_inc, expo_inc, tex, keep, n, steps, step_of_row,
                             head_mask);
}
// Per-image seeds: one workgroup per image runs the loop above on the image's
// own T rows with the image's own seed from generator offset 0 -- what t2h_unmask_schedule[_keep] writes for a batch that
// holds this image alone.  The steps are sequential and the images independent: the launch takes as long as one image.
template <bool KEEP>
__global__ __launch_bounds__(SCHED_THREADS) void unmask_schedule_batch_kernel(
    const uint64_t* __restrict__ seeds, uint32_t rand_grid_threads, uint32_t rand_inc, uint32_t expo_inc,
    const int64_t* __restrict__ tex, const uint8_t* __restrict__ keep, int T, int steps,
    int32_t* __restrict__ step_of_row, uint32_t* __restrict__ head_mask) {
  const int64_t r0 = (int64_t)blockIdx.x * T;
  unmask_schedule_rows<KEEP>(seeds[blockIdx.x], 0, rand_grid_threads, rand_inc, expo_inc, tex + r0,
                             KEEP ? keep + r0 : nullptr, T, steps, step_of_row + r0,
                             head_mask + (int64_t)blockIdx.x * (steps + 1));
}

// ---- region editing: the reference loop started from a partially known state ("Editing a region").
// Prefill: kept rows (keep[i] != 0) start as their source token src[tex[i]][i] (+ n_class * tex[i] in x_t), every
// other row masked; out_lists[h][i] = the kept token where h == tex[i], else -1.  A kept row without a valid source
// token under its texture (-1, or outside [0, n_class)) raises the error word: err = max(err, n - i), so the host reads
// the FIRST such row as n - err (err == 0: none; the host zeroes it).  x_t / out_lists may be NULL (check only).
__global__ void edit_prefill_kernel(const int64_t* __restrict__ src, const int64_t* __restrict__ tex,
                                    const uint8_t* __restrict__ keep, int64_t mask_id, int64_t* __restrict__ x_t,
                                    int64_t* __restrict__ out, uint32_t* __restrict__ err, int n, int n_heads,
                                    int n_class) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int h = (int)tex[i];
  const bool k = keep[i] != 0;
  const int64_t v = (k && h >= 0 && h < n_heads) ? src[(int64_t)h * n + i] : -1;
  const bool ok = v >= 0 && v < n_class;
  if (k && !ok) atomicMax(err, (uint32_t)(n - i));
  const bool kept = k && ok;
  if (x_t) x_t[i] = kept ? v + (int64_t)n_class * h : mask_id;
  if (out)
    for (int j = 0; j < n_heads; ++j) out[(int64_t)j * n + i] = (kept && j == h) ? v : -1;
}

// Region -> keep: one wave per token cell (th x tw cells of (H / th) x (W / tw) pixels); the cell is resampled
// (keep = 0) iff ANY of its pixels is in the region.  mode 0: uint8 mask, nonzero = region; mode 1: fp32 mask,
// nonzero = region; mode 2: fp32 parsing map, region = the labels whose bit is set in label_bits (ids 0..63).
constexpr int RK_CELLS = 4;  // cells (waves) per workgroup
__global__ __launch_bounds__(64 * RK_CELLS) void region_keep_kernel(const uint8_t* __restrict__ mask_u8,
                                                                  const float* __restrict__ map_f32,
                                                                  uint64_t label_bits, int mode, int H, int W, int th,
                                                                  int tw, int n_cells, uint8_t* __restrict__ keep) {
  const int lane = threadIdx.x & 63;
  const int cell = blockIdx.x * RK_CELLS + (threadIdx.x >> 6);
  if (cell >= n_cells) return;  // (uniform over the wave)
  const int T = th * tw, b = cell / T, c = cell - b * T, ci = c / tw, cj = c - ci * tw;
  const int ch = H / th, cw = W / tw;
  int hit = 0;
  for (int p = lane; p < ch * cw; p += 64) {
    const int y = ci * ch + p / cw, x = cj * cw + p % cw;
    const int64_t q = ((int64_t)b * H + y) * W + x;
    if (mode == 0) {
      hit |= mask_u8[q] != 0;
    } else if (mode == 1) {
      hit |= map_f32[q] != 0.f;
    } else {
      const float v = map_f32[q];
      const int l = (int)v;
      hit |= (v >= 0.f && v < 64.f && (float)l == v && ((label_bits >> l) & 1ull)) ? 1 : 0;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) hit |= __shfl_xor(hit, o, 64);
  if (lane == 0) keep[cell] = hit ? 0 : 1;
}

// dst[h][r] = src[h][r] where keep[r] (bottom indices of an edited photo: the encoder's outside the region)
__global__ void merge_kept_kernel(const int64_t* __restrict__ src, const uint8_t* __restrict__ keep,
                                  int64_t* __restrict__ dst, int n, int64_t total) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  if (keep[i % n]) dst[i] = src[i];
}

// ---- self-correction: the fold lattice of the pseudo-likelihood critic, the choice of the rows to
// redo and the per-image accept.
// The fold of token row i of a th x tw map (r = i / tw, c = i % tw): K = 2 a checkerboard, K = 4 / 8 / 16 lattices on
// which no two 8-neighbours share a fold.
__device__ __forceinline__ int fold_of_row(int i, int tw, int K) {
  const int r = i / tw, c = i - r * tw;
  return K == 2 ? (r + c) & 1 : K == 4 ? (r & 1) * 2 + (c & 1) : K == 8 ? (r & 3) * 2 + (c & 1) : (r & 3) * 4 + (c & 3);
}

// keep_k[k][b][i] = 1 iff row i is not in fold k, or the caller keeps it (keep may be NULL)
__global__ void fold_keep_kernel(const uint8_t* __restrict__ keep, int K, int n, int T, int tw,
                                 uint8_t* __restrict__ keep_k, int64_t total) {
  const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= total) return;
  const int k = (int)(q / n), j = (int)(q - (int64_t)k * n);
  keep_k[q] = (fold_of_row(j % T, tw, K) != k || (keep && keep[j] != 0)) ? 1 : 0;
}

// out[j] = src_k[fold(j)][j]: every row from the evaluation that hid it (logp, and rank where given)
__global__ void fold_gather_kernel(const float* __restrict__ logp_k, const int32_t* __restrict__ rank_k, int K, int n,
                                   int T, int tw, float* __restrict__ logp, int32_t* __restrict__ rank) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const int64_t q = (int64_t)fold_of_row(j % T, tw, K) * n + j;
  logp[j] = logp_k[q];
  if (rank) rank[j] = rank_k[q];
}

// The count[b] rows of image b with the lowest score get keep_out = 0 (redo), every other row 1.  A row is eligible iff
// its score is not NaN; the order is ascending by value (<, ==: -inf is the smallest, +0 and -0 tie), ties by the lower
// row index.  One workgroup per image, the scores in LDS; a row's place in the order is counted, not sorted, so the
// result does not depend on the thread count.
constexpr int SEL_THREADS = 256, SEL_MAX_T = 1024;
__global__ __launch_bounds__(SEL_THREADS) void select_lowest_kernel(const float* __restrict__ score,
                                                                   const int32_t* __restrict__ count, int T,
                                                                   uint8_t* __restrict__ keep_out,
                                                                   int32_t* __restrict__ n_sel) {
  __shared__ float s_s[SEL_MAX_T];
  __shared__ int red[SEL_THREADS / 64];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* sc = score + (int64_t)b * T;
  int elig = 0;
  for (int i = tid; i < T; i += SEL_THREADS) {
    const float v = sc[i];
    s_s[i] = v;
    elig += v == v ? 1 : 0;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) elig += __shfl_xor(elig, o, 64);
  if (lane == 0) red[wave] = elig;
  __syncthreads();
  elig = 0;
  for (int k = 0; k < SEL_THREADS / 64; ++k) elig += red[k];
  const int want = count[b] > 0 ? count[b] : 0;
  const int m = want < elig ? want : elig;
  for (int i = tid; i < T; i += SEL_THREADS) {
    const float si = s_s[i];
    int before = 0;
    for (int j = 0; j < T; ++j) {
      const float sj = s_s[j];
      before += (sj < si || (sj == si && j < i)) ? 1 : 0;  // (a NaN compares false both ways: never before anything)
    }
    keep_out[(int64_t)b * T + i] = (si == si && before < m) ? 0 : 1;
  }
  if (tid == 0) n_sel[b] = m;
}

// Image b takes the candidate -- its n_heads index lists and its scores -- iff always, or sum_cand[b] > sum_cur[b]
// (strictly: an equal sum, a -inf candidate and a NaN keep the current map).  sum_out[b] / accepted[b]: the sum the image
// now has, and whether it took the candidate; sum_cur is only read.
__global__ void accept_merge_kernel(const int64_t* __restrict__ cand, const float* __restrict__ cand_score,
                                    const float* __restrict__ sum_cand, const float* __restrict__ sum_cur, int always,
                                    int64_t* __restrict__ cur, float* __restrict__ cur_score,
                                    float* __restrict__ sum_out, uint8_t* __restrict__ accepted, int B, int T,
                                    int64_t total) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int n = B * T, j = (int)(i % n), b = j / T;
  const bool take = always || sum_cand[b] > sum_cur[b];
  if (take) cur[i] = cand[i];
  if (i < n && take) cur_score[i] = cand_score[i];
  if (i < B) {
    const bool tb = always || sum_cand[i] > sum_cur[i];
    sum_out[i] = tb ? sum_cand[i] : sum_cur[i];
    accepted[i] = tb ? 1 : 0;
  }
}

// ---- round cursor of a pre-computed schedule (engine.sample_tokens, graph replay): copies round
// r = *round_ctr of the padded [rounds][maxr] tables into fixed staging buffers and advances the
// counter, so that every round of a sampling run is the SAME launch sequence with the same arguments
// (capturable once, replayed per round) while the rows / generator offsets it works on change.
__global__ void schedule_advance_kernel(const int32_t* __restrict__ rows_tbl, const int64_t* __restrict__ aux64_tbl,
                                        const int32_t* __restrict__ aux32_tbl, int32_t* __restrict__ round_ctr,
                                        int32_t* __restrict__ cur_rows, int64_t* __restrict__ cur_aux64,
                                        int32_t* __restrict__ cur_aux32, int maxr) {
  const int r = *round_ctr;
  for (int i = threadIdx.x; i < maxr; i += blockDim.x) {
    const int64_t j = (int64_t)r * maxr + i;
    cur_rows[i] = rows_tbl[j];
    if (aux64_tbl) cur_aux64[i] = aux64_tbl[j];
    if (aux32_tbl) cur_aux32[i] = aux32_tbl[j];
  }
  __syncthreads();  // every thread has read r
  if (threadIdx.x == 0) *round_ctr = r + 1;
}

// ---- two-launch form of the same tail (t2h_sample_heads with a logits workspace).  One workgroup
// per changed row streams 2 MB of head weights by itself (~50 us per step with ~16 rows on 16 CUs);
// here SL_SPLIT workgroups per row take n_class / SL_SPLIT classes each (LN_f recomputed per
// workgroup: 2 KB), then a second launch does max / exponential race over the row's logits.
// Both forms take every logit from head_dot4 and draw through the same row_max / row_theta / race, so the results
// are bit-identical to the one-launch form.
constexpr int SL_SPLIT = 8, SL_THREADS = 256;

template <int C, bool PER_SAMPLE>
__global__ __launch_bounds__(SL_THREADS) void sample_logits_kernel(const t2h_sample_heads_args a, float* __restrict__ ws,
                                                                   const t2h_sample_params* __restrict__ params, int T) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int slot = blockIdx.x / SL_SPLIT, part = blockIdx.x - slot * SL_SPLIT;
  const int row = a.rows[slot];
  const int head = (int)a.tex[row];
  f32x4 v[C / 256];
  lnf_row<C>(a.hidden + (int64_t)(a.hidden_compact ? slot : row) * C, a.lnf_gamma, a.lnf_beta, lane, v);
  const float temp = PER_SAMPLE ? params[row / T].temp : a.temp;
  const float* w = a.w_heads + (int64_t)head * a.n_class * C;
  const int per = (a.n_class + SL_SPLIT - 1) / SL_SPLIT;
  const int j_end = min(a.n_class, (part + 1) * per);
  constexpr int NW = SL_THREADS / 64;
  for (int j0 = part * per + wave * 4; j0 < j_end; j0 += NW * 4) {
    float acc[4];
    head_dot4<C>(w, j0, a.n_class, lane, v, acc);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const float r = wave_sum(acc[u]);
      if (lane == 0 && j0 + u < j_end) ws[(int64_t)slot * a.n_class + j0 + u] = r / temp;  // (divides, like the reference)
    }
  }
}

// SEEDED (per-image seeds): the seed of row `row` is philox_seed_img[row / img_rows] and its noise row,
// unless rng_rows names one, row % img_rows -- the image's own stream, whatever batch it sits in.  The SEEDED = false
// instances are the code without either.
template <bool SEEDED, bool TRUNC, bool PER_SAMPLE, bool LOGP>
__global__ __launch_bounds__(SH_THREADS) void sample_pick_kernel(const t2h_sample_heads_args a, const float* __restrict__ ws,
                                                                 const t2h_sample_params* __restrict__ params, int T) {
  __shared__ float red[2 * (SH_THREADS / 64)];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  constexpr int NW = SH_THREADS / 64;
  const int slot = blockIdx.x, row = a.rows[slot];
  const int head = (int)a.tex[row];
  const float* lg = ws + (int64_t)slot * a.n_class;
  const float mx = row_max<SH_THREADS>(lg, a.n_class, tid, red, lane, wave);
  const sample_settings st = row_settings<PER_SAMPLE>(a.temp, a.top_k, a.top_p_q, params, row, T, a.n_class);
  const float theta = row_theta<SH_THREADS, TRUNC, PER_SAMPLE>(lg, a.n_class, mx, st.top_k, st.top_p_q, tid);
  // noise of this row: explicit compact rows (expo_rows[expo_slot[slot]]), the head's explicit full
  // tensor, or computed -- at the row's own generator offset when the list mixes steps
  const float* er = a.expo_rows ? a.expo_rows + (int64_t)(a.expo_slot ? a.expo_slot[slot] : slot) * a.n_class
                    : a.philox_grid_threads ? nullptr
                                            : a.expo[head] + (int64_t)row * a.n_class;
  const uint64_t poff = a.row_philox_offset ? a.row_philox_offset[slot] : a.philox_offset[head];
  const uint64_t pseed = SEEDED              ? a.philox_seed_img[row / a.img_rows]  // (row is uniform: one scalar load)
                         : a.philox_seed_dev ? *a.philox_seed_dev
                                             : a.philox_seed;
  // the element of the reference's [n, n_class] draw this row owns: its row THERE (the host may have reordered the
  // samples of the batch, rng_rows) -- by default the row itself, SEEDED: its row in its own image's [T, n_class] draw
  const int rng_row = a.rng_rows ? a.rng_rows[slot] : SEEDED ? row % a.img_rows : row;
  race best;
  for (int j = tid; j < a.n_class; j += SH_THREADS) {
    if (TRUNC && !(lg[j] >= theta)) continue;
    const float q = er ? er[j]
                       : torch_exponential_at(pseed, poff, a.philox_grid_threads,
                                              (uint64_t)rng_row * a.n_class + j);
    best.offer(expf(lg[j] - mx) / q, j);
  }
  best.wave_reduce();
  best.block_reduce<NW>(red, reinterpret_cast<int*>(red + NW), tid);
  if (tid == 0) {
    a.x_t[row] = (int64_t)best.winner(a.n_class) + (int64_t)a.n_class * head;
    a.out_idx[(int64_t)head * a.n + row] = best.winner(a.n_class);
  }
  if constexpr (LOGP) {  // (after the race: its barrier frees red[] once thread 0 has read the winner)
    const float se = row_logsum<SH_THREADS>(lg, a.n_class, mx, tid, red, lane, wave);
    if (tid == 0) a.logp[row] = (lg[best.winner(a.n_class)] - mx) - logf(se);
  }
}

// ---- scoring a given token map: the second launch of the two-launch tail with the row's token READ
// from targets[head][row] instead of raced for.  The log-probability is formed by the functions, in the order, of the LOGP
// tail above (row_max, row_logsum, then (l_tok - max) - logf(se) on thread 0), so a token that sample_pick_kernel drew
// scores the bits that launch wrote.  rank = the number of classes with a strictly greater logit: an integer count (wave
// butterfly, the waves through LDS), so it does not depend on any order.  No noise is read.  A token outside
// [0, n_class) indexes nothing: logp = NaN, rank = -1, x_t / out_idx untouched.
__global__ __launch_bounds__(SH_THREADS) void score_pick_kernel(const t2h_sample_heads_args a, const float* __restrict__ ws,
                                                                const int64_t* __restrict__ targets,
                                                                int32_t* __restrict__ rank) {
  constexpr int NW = SH_THREADS / 64;
  __shared__ float red[NW];
  __shared__ int cnt[NW];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int slot = blockIdx.x, row = a.rows[slot];
  const int head = (int)a.tex[row];
  const int64_t tok = targets[(int64_t)head * a.n + row];
  if (tok < 0 || tok >= a.n_class) {  // (uniform over the workgroup: nobody reaches a barrier)
    if (tid == 0) {
      a.logp[row] = __builtin_nanf("");
      if (rank) rank[row] = -1;
    }
    return;
  }
  const float* lg = ws + (int64_t)slot * a.n_class;
  const float mx = row_max<SH_THREADS>(lg, a.n_class, tid, red, lane, wave);
  const float se = row_logsum<SH_THREADS>(lg, a.n_class, mx, tid, red, lane, wave);
  const float lt = lg[tok];
  if (tid == 0) {
    a.logp[row] = (lt - mx) - logf(se);
    a.x_t[row] = tok + (int64_t)a.n_class * head;
    a.out_idx[(int64_t)head * a.n + row] = tok;
  }
  if (rank) {  // (uniform over the workgroup)
    int c = 0;
    for (int j = tid; j < a.n_class; j += SH_THREADS) c += lg[j] > lt ? 1 : 0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    if (lane == 0) cnt[wave] = c;
    __syncthreads();
    if (tid == 0) {
      int tot = 0;
      for (int k = 0; k < NW; ++k) tot += cnt[k];
      rank[row] = tot;
    }
  }
}

// All heads in one launch: one workgroup per CHANGED token (compact list from
// unmask_step), which picks the head / noise tensor of its own texture.
template <int C, bool TRUNC, bool PER_SAMPLE, bool LOGP>
__global__ __launch_bounds__(SH_THREADS) void sample_heads_kernel(const t2h_sample_heads_args a,
                                                                  const t2h_sample_params* __restrict__ params, int T) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int row = a.rows[blockIdx.x];
  const int head = (int)a.tex[row];
  const float* expo = a.expo[head];
  if (expo == nullptr) return;  // cannot happen: a head with changed tokens always drew its noise
  const sample_settings st = row_settings<PER_SAMPLE>(a.temp, a.top_k, a.top_p_q, params, row, T, a.n_class);
  sample_row<C, TRUNC, PER_SAMPLE, LOGP>(lds, row, a.hidden, a.lnf_gamma, a.lnf_beta,
                                         a.w_heads + (int64_t)head * a.n_class * C, expo, head, st.temp, a.x_t,
                                         a.out_idx + (int64_t)head * a.n, a.n_class, st.top_k, st.top_p_q,
                                         a.logp);  // (full hidden only)
}

// ---- confidence-ordered parallel decoding ("Confidence-ordered decoding").  A round samples EVERY masked
// row -- up to B * 512 rows instead of a few dozen -- so the head GEMV of the tail above (2 MB of weights per row) is
// the wrong shape: the masked rows are grouped by head, CT_ROWS rows of one head share one stream of its weights.
// Every logit is still wave_sum(lane_dot) over the lnf_row'ed row (which now comes from LDS instead of registers), so the
// logits, and the token the race draws, are the bits of t2h_sample_heads.
constexpr int CT_ROWS = 16, CT_SPLIT = 4, CT_THREADS = 256, CT_HDR = 4;

__host__ __device__ inline int conf_max_tiles(int n, int n_heads) { return (n + CT_ROWS - 1) / CT_ROWS + n_heads; }

// group_ws: [0] = number of tiles, [1] = number of masked rows, tiles {head, first slot, rows} from CT_HDR on, then the
// masked rows sorted by head.  (The order of a head's rows is whatever the atomics give: no result depends on it.)
__global__ __launch_bounds__(1024) void conf_group_kernel(const int64_t* __restrict__ x_t, const int64_t* __restrict__ tex,
                                                          int64_t mask_id, int n, int n_heads, int32_t* __restrict__ ws) {
  __shared__ int cnt[T2H_MAX_HEADS], first[T2H_MAX_HEADS], cur[T2H_MAX_HEADS];
  const int tid = threadIdx.x;
  const int max_tiles = conf_max_tiles(n, n_heads);
  int32_t* tiles = ws + CT_HDR;
  int32_t* rows = tiles + 3 * max_tiles;
  if (tid < T2H_MAX_HEADS) cnt[tid] = cur[tid] = 0;
  __syncthreads();
  for (int e = tid; e < n; e += blockDim.x) {
    const int h = (int)tex[e];
    if (x_t[e] == mask_id && h >= 0 && h < n_heads) atomicAdd(&cnt[h], 1);
  }
  __syncthreads();
  if (tid == 0) {
    int s = 0, t = 0;
    for (int h = 0; h < n_heads; ++h) {
      first[h] = s;
      for (int o = 0; o < cnt[h] && t < max_tiles; o += CT_ROWS, ++t) {
        tiles[3 * t] = h;
        tiles[3 * t + 1] = s + o;
        tiles[3 * t + 2] = min(CT_ROWS, cnt[h] - o);
      }
      s += cnt[h];
    }
    ws[0] = t;
    ws[1] = s;
  }
  __syncthreads();
  for (int e = tid; e < n; e += blockDim.x) {
    const int h = (int)tex[e];
    if (x_t[e] == mask_id && h >= 0 && h < n_heads) rows[first[h] + atomicAdd(&cur[h], 1)] = e;
  }
}

// One workgroup per (tile, class quarter): LN_f of the tile's rows into LDS (one wave per row), then every wave streams
// 4 weight rows at a time and uses them for all rows of the tile.
// PER_SAMPLE: the rows of a tile share a head, not an image -- the temperature is per ROW of the tile (lane r of
// every wave holds row r's, read back with v_readlane: no LDS beyond xs, whose 32 KiB fit five times into a CU's).
template <int C, bool PER_SAMPLE>
__global__ __launch_bounds__(CT_THREADS) void conf_logits_kernel(const t2h_confidence_tail_args a,
                                                                 const t2h_sample_params* __restrict__ params, int T) {
  constexpr int VPL = C / 256, NW = CT_THREADS / 64;
  __shared__ __attribute__((aligned(16))) float xs[CT_ROWS * C];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int tile = blockIdx.x / CT_SPLIT, part = blockIdx.x - tile * CT_SPLIT;
  const int32_t* ws = a.group_ws;
  if (tile >= ws[0]) return;  // (uniform over the workgroup)
  const int32_t* td = ws + CT_HDR + 3 * tile;
  const int head = td[0], cnt = min(td[2], CT_ROWS);
  const int32_t* rows = ws + CT_HDR + 3 * conf_max_tiles(a.n, a.n_heads) + td[1];
  for (int r = wave; r < cnt; r += NW) {
    f32x4 v[VPL];
    lnf_row<C>(a.hidden + (int64_t)rows[r] * C, a.lnf_gamma, a.lnf_beta, lane, v);
#pragma unroll
    for (int i = 0; i < VPL; ++i) *reinterpret_cast<f32x4*>(xs + r * C + i * 256 + lane * 4) = v[i];
  }
  __syncthreads();
  const float temp = a.temp;
  float row_temp = 1.f;
  if constexpr (PER_SAMPLE) {
    if (lane < cnt) row_temp = params[rows[lane] / T].temp;
  }
  const float* w = a.w_heads + (int64_t)head * a.n_class * C;
  const int per = (a.n_class + CT_SPLIT - 1) / CT_SPLIT;
  const int j_end = min(a.n_class, (part + 1) * per);
  for (int j0 = part * per + wave * 4; j0 < j_end; j0 += NW * 4) {
    f32x4 ww[4][VPL];
#pragma unroll
    for (int u = 0; u < 4; ++u) load_row(w + (int64_t)min(j0 + u, a.n_class - 1) * C, lane, ww[u]);
    for (int r = 0; r < cnt; ++r) {
      f32x4 v[VPL];
      load_row(xs + r * C, lane, v);
      float acc[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) acc[u] = lane_dot(ww[u], v);
      float* lg = a.logits_ws + (int64_t)rows[r] * a.n_class;
      const float tr = PER_SAMPLE ? __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, row_temp), r))
                                  : temp;
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const float res = wave_sum(acc[u]);
        if (lane == 0 && j0 + u < j_end) lg[j0 + u] = res / tr;
      }
    }
  }
}

// One wave per row: max, the exponential race at the wave's scope (same scores, lowest index of the maximum), the sum
// of the same exponentials, and the log-probability of the drawn class.
template <bool TRUNC, bool PER_SAMPLE>
__global__ __launch_bounds__(64 * CP_ROWS) void conf_pick_kernel(const t2h_confidence_tail_args a,
                                                                 const t2h_sample_params* __restrict__ params, int T) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * CP_ROWS + (threadIdx.x >> 6);
  if (row >= a.n) return;  // (uniform over the wave)
  const int head = (int)a.tex[row];
  if (a.x_t[row] != a.mask_id || head < 0 || head >= a.n_heads) {
    if (lane == 0) {
      a.tok[row] = -1;
      a.conf[row] = -INFINITY;
    }
    return;
  }
  const float* lg = a.logits_ws + (int64_t)row * a.n_class;
  const float mx = row_max<64>(lg, a.n_class, lane, nullptr, lane, 0);
  const sample_settings st =
      row_settings<PER_SAMPLE>(a.temp, a.top_k, a.top_p_q, params, __builtin_amdgcn_readfirstlane(row), T, a.n_class);
  // only the token changes: se / conf below stay those of the full softmax
  const float theta = row_theta<64, TRUNC, PER_SAMPLE>(lg, a.n_class, mx, st.top_k, st.top_p_q, lane);
  const float* er = a.expo ? a.expo + (int64_t)row * a.n_class : nullptr;
  const uint64_t pseed = a.philox_seed_dev ? *a.philox_seed_dev : a.philox_seed;
  const uint64_t poff = a.philox_offset_dev ? *a.philox_offset_dev : a.philox_offset;
  race best;
  float se = 0.f;
  for (int j = lane; j < a.n_class; j += 64) {
    const float q = er ? er[j] : torch_exponential_at(pseed, poff, a.philox_grid_threads, (uint64_t)row * a.n_class + j);
    const float ex = expf(lg[j] - mx);
    const float sc = ex / q;
    se += ex;
    if (TRUNC && !(lg[j] >= theta)) continue;
    best.offer(sc, j);
  }
  best.wave_reduce();
  se = wave_sum(se);
  if (lane == 0) {
    const int tok = best.winner(a.n_class);
    a.tok[row] = tok;
    a.conf[row] = (lg[tok] - mx) - logf(se);
  }
}

// One workgroup per sample: scores into LDS, rank of every masked row by counting, the k best commit.
constexpr int CC_THREADS = 512, CC_MAX_T = 2048;
__device__ __forceinline__ bool conf_before(float sj, int j, float si, int i) {  // row j ranks before row i
  const bool nj = sj != sj, ni = si != si;
  if (nj || ni) return nj == ni ? j < i : ni;
  return sj > si || (sj == si && j < i);
}
template <bool PER_SAMPLE>  // PER_SAMPLE: a.tau is [B], the sample's own choice temperature
__global__ __launch_bounds__(CC_THREADS) void conf_commit_kernel(const t2h_confidence_commit_args a) {
  __shared__ float s_s[CC_MAX_T];
  __shared__ int m_s[CC_MAX_T];
  const int b = blockIdx.x, tid = threadIdx.x, T = a.T;
  const int k = a.k[b];
  const float tau = PER_SAMPLE ? a.tau[b] : *a.tau;
  const uint64_t pseed = a.philox_seed_dev ? *a.philox_seed_dev : a.philox_seed;
  const uint64_t poff = a.philox_offset_dev ? *a.philox_offset_dev : a.philox_offset;
  for (int i = tid; i < T; i += CC_THREADS) {
    const int64_t row = (int64_t)b * T + i;
    const int64_t h = a.tex[row];
    const bool masked = a.x_t[row] == a.mask_id && a.tok[row] >= 0 && a.tok[row] < a.n_class && h >= 0 && h < a.n_heads;
    float s = -INFINITY;
    if (masked) {
      float u = a.u ? a.u[row] : torch_uniform_at(pseed, poff, a.philox_grid_threads, (uint64_t)row);
      u = fminf(fmaxf(u, 5.9604644775390625e-8f), 1.0f - 5.9604644775390625e-8f);
      const float g = -logf(-logf(u));
      s = __fadd_rn(a.conf[row], __fmul_rn(tau, g));
    }
    s_s[i] = s;
    m_s[i] = masked ? 1 : 0;
    if (a.scores) a.scores[row] = s;
  }
  __syncthreads();
  for (int i = tid; i < T; i += CC_THREADS) {
    if (!m_s[i]) continue;
    const float si = s_s[i];
    int rank = 0;
    for (int j = 0; j < T; ++j) rank += (m_s[j] && j != i && conf_before(s_s[j], j, si, i)) ? 1 : 0;
    if (rank < k) {
      const int64_t row = (int64_t)b * T + i;
      const int64_t tk = a.tok[row], h = a.tex[row];
      a.x_t[row] = tk + (int64_t)a.n_class * h;
      a.out[h * ((int64_t)a.B * T) + row] = tk;
      if (a.logp) a.logp[row] = a.conf[row];  // (a copy: the log-probability the tail formed for the committed token)
    }
  }
}

// ---- t2h_logp_summary: per image, the sum / count / minimum of the log-probabilities of its drawn rows (NaN = never
// drawn: skipped).  One workgroup per image on a tree that depends on T alone: thread t takes rows t, t + 256, ... in
// ascending order, then the wave butterfly, then the four waves in wave order -- an image's three numbers do not depend
// on where it sits in the batch.
constexpr int LS_THREADS = 256;
__global__ __launch_bounds__(LS_THREADS) void logp_summary_kernel(const float* __restrict__ logp, int T,
                                                                  float* __restrict__ sum, int32_t* __restrict__ count,
                                                                  float* __restrict__ mn) {
  constexpr int NW = LS_THREADS / 64;
  __shared__ float red_s[NW], red_m[NW];
  __shared__ int red_c[NW];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* lp = logp + (int64_t)b * T;
  float s = 0.f, m = INFINITY;
  int c = 0;
  for (int i = tid; i < T; i += LS_THREADS) {
    const float v = lp[i];
    if (v != v) continue;
    s += v;
    m = fminf(m, v);
    ++c;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    s += __shfl_xor(s, o, 64);
    m = fminf(m, __shfl_xor(m, o, 64));
    c += __shfl_xor(c, o, 64);
  }
  if (lane == 0) {
    red_s[wave] = s;
    red_m[wave] = m;
    red_c[wave] = c;
  }
  __syncthreads();
  if (tid == 0) {
    for (int k = 1; k < NW; ++k) {
      s += red_s[k];
      m = fminf(m, red_m[k]);
      c += red_c[k];
    }
    sum[b] = s;
    count[b] = c;
    mn[b] = m;
  }
}

// ---- t2h_truncation_threshold: the selection alone, at the scope of sample_pick_kernel (one workgroup per row) or of
// conf_pick_kernel (one wave per row), with their row_max.
template <int NT, bool PER_SAMPLE>
__global__ __launch_bounds__(NT == 64 ? 64 * CP_ROWS : SH_THREADS) void trunc_threshold_kernel(
    const float* __restrict__ logits, int n_rows, int n_class, int top_k, uint32_t top_p_q, float* __restrict__ theta,
    int* __restrict__ kept, const t2h_sample_params* __restrict__ params, int T) {
  constexpr int ROWS = NT == 64 ? CP_ROWS : 1;
  __shared__ trunc_lds tr[ROWS];
  __shared__ float red[SH_THREADS / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int row = NT == 64 ? blockIdx.x * CP_ROWS + wave : blockIdx.x;
  if (row >= n_rows) return;  // (uniform over the wave; the workgroup form has one row per workgroup)
  const int t = NT == 64 ? lane : (int)threadIdx.x;
  const sample_settings st =
      row_settings<PER_SAMPLE>(0.f, top_k, top_p_q, params, __builtin_amdgcn_readfirstlane(row), T, n_class);
  const bool cut = st.top_k != 0 || st.top_p_q != 0;
  const float* lg = logits + (int64_t)row * n_class;
  const float mx = row_max<NT>(lg, n_class, t, red, lane, wave);
  int n_kept = n_class;
  uint32_t key = 0;
  if (cut) key = trunc_select<NT>(lg, n_class, mx, st.top_k, st.top_p_q, &tr[NT == 64 ? wave : 0], t, &n_kept);
  if (t == 0) {
    theta[row] = cut ? trunc_unkey(key) : -INFINITY;
    kept[row] = n_kept;
  }
}

// ---- sampled bottom-index refinement: routed_head_argmax_kernel of vq.hip with a draw in place of the
// maximum.  One workgroup per token, the token's Cf features in LDS, thread t owns classes t, t + 256, ...: the logit of
// a class is that kernel's serial fma chain + bias (the same float), divided by the temperature into LDS; then the row
// maximum, the threshold of truncated sampling (the workgroup form of trunc_select) and the race, noise
// explicit or element (noise_row0 + row, j) of torch's whole-tensor exponential_ draw.
constexpr int RS_THREADS = 256;
template <bool TRUNC, bool PER_SAMPLE>
__global__ __launch_bounds__(RS_THREADS) void routed_head_sample_kernel(const t2h_routed_sample_args a,
                                                                        const t2h_sample_params* __restrict__ params,
                                                                        int T) {
  extern __shared__ __attribute__((aligned(16))) float lds[];  // Cf features, n_class logits, 3 * NW reduce slots
  constexpr int NW = RS_THREADS / 64;
  const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  float* fs = lds;
  float* lg = lds + a.Cf;
  float* red = lg + a.n_class;
  const int64_t tex = a.tex[row];
  for (int hd = tid; hd < a.n_heads; hd += RS_THREADS)
    if (hd != tex) a.out_lists[(int64_t)hd * a.n + row] = -1;
  if (tex < 0 || tex >= a.n_heads) {  // (uniform over the workgroup)
    if (tid == 0 && a.logp) a.logp[row] = -INFINITY;
    return;
  }
  const int t = (int)tex;
  const sample_settings st = row_settings<PER_SAMPLE>(a.temp, a.top_k, a.top_p_q, params, row, T, a.n_class);
  for (int k = tid; k < a.Cf; k += RS_THREADS) fs[k] = a.feat[(int64_t)row * a.ldf + t * a.Cf + k];
  __syncthreads();
  float mx = -INFINITY;
  for (int j = tid; j < a.n_class; j += RS_THREADS) {
    const float* wr = a.w + ((int64_t)t * a.n_class + j) * a.Cf;
    float acc = 0.f;
    for (int k = 0; k < a.Cf; ++k) acc = fmaf(wr[k], fs[k], acc);
    acc += a.b[t * a.n_class + j];
    const float l = acc / st.temp;
    lg[j] = l;
    if (a.logits_ws) a.logits_ws[(int64_t)row * a.n_class + j] = l;
    mx = fmaxf(mx, l);
  }
  mx = block_max<RS_THREADS>(mx, red, lane, wave);  // (its barrier also publishes lg[]: every logit of the row is in LDS)
  // only the token changes: se / logp below stay those of the full softmax
  const float theta = row_theta<RS_THREADS, TRUNC, PER_SAMPLE>(lg, a.n_class, mx, st.top_k, st.top_p_q, tid);
  const float* er = a.expo ? a.expo + (int64_t)row * a.n_class : nullptr;
  const uint64_t e0 = (uint64_t)(a.noise_row0 + row) * (uint64_t)a.n_class;
  race best;
  float se = 0.f;
  for (int j = tid; j < a.n_class; j += RS_THREADS) {
    const float q = er ? er[j] : torch_exponential_at(a.philox_seed, a.philox_offset, a.philox_grid_threads, e0 + j);
    const float ex = expf(lg[j] - mx);
    const float sc = ex / q;
    se += ex;
    if (TRUNC && !(lg[j] >= theta)) continue;
    best.offer(sc, j);
  }
  best.wave_reduce();
  se = wave_sum(se);
  float* reds = red + NW;
  if (lane == 0) reds[wave] = se;  // (slots of its own: published by block_reduce's barriers)
  best.block_reduce<NW>(red, reinterpret_cast<int*>(red + 2 * NW), tid);
  if (tid == 0) {
    se = reds[0];
    for (int k = 1; k < NW; ++k) se += reds[k];
    const int tok = best.winner(a.n_class);
    a.out_lists[(int64_t)t * a.n + row] = tok;
    if (a.logp) a.logp[row] = (lg[tok] - mx) - logf(se);
  }
}
}  // namespace

// top_k >= n_class and top_p_q == 2^20 cut nothing: off (the existing kernels)
static inline bool trunc_settings(int32_t n_class, int32_t* top_k, uint32_t* top_p_q) {
  if (*top_k >= n_class) *top_k = 0;
  if (*top_p_q == (1u << 20)) *top_p_q = 0;
  return *top_k != 0 || *top_p_q != 0;
}
#define T2H_TRUNC_REQUIRE(name, a_top_k, a_top_p_q, a_n_class)                                                         \
  T2H_REQUIRE((a_top_k) >= 0 && (a_top_p_q) <= (1u << 20) && ((a_top_p_q) == 0 || (a_n_class) <= 2048),                \
              name ": top_k=%d / top_p_q=%u out of range (top_k >= 0, top_p_q <= 2^20; top-p: n_class <= 2048)",     \
              (int)(a_top_k), (unsigned)(a_top_p_q))

// A per-sample table sits in device memory: its VALUES are the caller's to validate (ops.sampling_params); the kernels
// treat anything that cuts nothing as off.  Any image may use top-p, so its class limit holds for the whole launch.
#define T2H_PER_SAMPLE_REQUIRE(name, params, T, n, a_n_class)                                                          \
  T2H_REQUIRE((params) != nullptr && (T) > 0 && (n) % (T) == 0 && (a_n_class) <= 2048,                                 \
              name ": params[n / rows_per_sample] expected, rows_per_sample=%d dividing n=%d; n_class <= 2048", (int)(T), \
              (int)(n))

// The instance of a <[...,] TRUNC, PER_SAMPLE> tail kernel for a launch: PER_SAMPLE for a table (`params`), else the
// scalars' instance with or without the truncation code (`trunc`).  Leading template arguments follow the name.
#define T2H_TAIL_KERNEL(kernel, ...)                                                                                  \
  (params ? kernel<__VA_ARGS__ true, true> : trunc ? kernel<__VA_ARGS__ true, false> : kernel<__VA_ARGS__ false, false>)
// The same for a <[...,] TRUNC, PER_SAMPLE, LOGP> kernel: the LOGP = false instances (the code without the log-sum) unless
// the launch has a `logp` output.
#define T2H_TAIL_KERNEL_L(kernel, LOGP, ...)                                                                          \
  (params  ? kernel<__VA_ARGS__ true, true, LOGP>                                                                     \
   : trunc ? kernel<__VA_ARGS__ true, false, LOGP>                                                                    \
           : kernel<__VA_ARGS__ false, false, LOGP>)
#define T2H_TAIL_KERNEL_LOGP(kernel, logp, ...) \
  ((logp) ? T2H_TAIL_KERNEL_L(kernel, true, __VA_ARGS__) : T2H_TAIL_KERNEL_L(kernel, false, __VA_ARGS__))

template <bool PER_SAMPLE>
static int trunc_threshold_launch(const float* logits, int32_t n_rows, int32_t n_class, int32_t top_k, uint32_t top_p_q,
                                  const t2h_sample_params* params, int32_t T, int32_t scope, float* theta, int32_t* kept,
                                  void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (scope == 0)
    hipLaunchKernelGGL((trunc_threshold_kernel<SH_THREADS, PER_SAMPLE>), dim3(n_rows), dim3(SH_THREADS), 0, s, logits,
                       n_rows, n_class, top_k, top_p_q, theta, kept, params, T);
  else
    hipLaunchKernelGGL((trunc_threshold_kernel<64, PER_SAMPLE>), dim3((n_rows + CP_ROWS - 1) / CP_ROWS), dim3(64 * CP_ROWS),
                       0, s, logits, n_rows, n_class, top_k, top_p_q, theta, kept, params, T);
  T2H_CHECK_LAUNCH("t2h_truncation_threshold");
  return T2H_OK;
}

extern "C" int t2h_truncation_threshold(const float* logits, int32_t n_rows, int32_t n_class, int32_t top_k,
                                        uint32_t top_p_q, int32_t scope, float* theta, int32_t* kept, void* stream) {
  T2H_REQUIRE(logits && theta && kept, "t2h_truncation_threshold: NULL pointer");
  T2H_REQUIRE(n_rows > 0 && n_class > 0 && (scope == 0 || scope == 1), "t2h_truncation_threshold: bad arguments");
  T2H_TRUNC_REQUIRE("t2h_truncation_threshold", top_k, top_p_q, n_class);
  trunc_settings(n_class, &top_k, &top_p_q);
  return trunc_threshold_launch<false>(logits, n_rows, n_class, top_k, top_p_q, nullptr, 0, scope, theta, kept, stream);
}

extern "C" int t2h_truncation_threshold_per_row(const float* logits, int32_t n_rows, int32_t n_class,
                                                const t2h_sample_params* params, int32_t rows_per_sample, int32_t scope,
                                                float* theta, int32_t* kept, void* stream) {
  T2H_REQUIRE(logits && theta && kept, "t2h_truncation_threshold_per_row: NULL pointer");
  T2H_REQUIRE(n_rows > 0 && n_class > 0 && (scope == 0 || scope == 1), "t2h_truncation_threshold_per_row: bad arguments");
  T2H_PER_SAMPLE_REQUIRE("t2h_truncation_threshold_per_row", params, rows_per_sample, n_rows, n_class);
  return trunc_threshold_launch<true>(logits, n_rows, n_class, 0, 0, params, rows_per_sample, scope, theta, kept, stream);
}

// params == NULL: the struct's scalars (the instance without truncation code where they cut nothing); else the
// PER_SAMPLE instance (a.temp / a.top_k / a.top_p_q are not read).  Nothing is launched on an error.
extern "C" int t2h_routed_head_sample(const t2h_routed_sample_args* args, const t2h_sample_params* params,
                                      int32_t rows_per_sample, void* stream) {
  T2H_REQUIRE(args != nullptr, "t2h_routed_head_sample: args is NULL");
  t2h_routed_sample_args a = *args;
  if (params) a.temp = 1.f, a.top_k = 0, a.top_p_q = 0;
  T2H_REQUIRE(a.feat && a.w && a.b && a.tex && a.out_lists, "t2h_routed_head_sample: NULL pointer");
  T2H_REQUIRE(a.n > 0 && a.n_heads > 0 && a.Cf > 0 && a.n_class > 0 && (int64_t)a.ldf >= (int64_t)a.n_heads * a.Cf,
              "t2h_routed_head_sample: bad shape (n=%d n_heads=%d Cf=%d n_class=%d ldf=%d)", a.n, a.n_heads, a.Cf,
              a.n_class, a.ldf);
  T2H_REQUIRE(a.temp > 0.f, "t2h_routed_head_sample: temp must be > 0");
  T2H_REQUIRE(a.expo != nullptr || (a.philox_grid_threads != 0 && a.philox_offset % 4 == 0 && a.noise_row0 >= 0),
              "t2h_routed_head_sample: no noise (expo, or philox_grid_threads, an offset that is a multiple of 4 and "
              "noise_row0 >= 0)");
  T2H_TRUNC_REQUIRE("t2h_routed_head_sample", a.top_k, a.top_p_q, a.n_class);
  if (params) T2H_PER_SAMPLE_REQUIRE("t2h_routed_head_sample", params, rows_per_sample, a.n, a.n_class);
  const size_t lds = ((size_t)a.Cf + a.n_class + 3 * (RS_THREADS / 64)) * sizeof(float);
  if (lds > 48 * 1024) {
    t2h_set_error("t2h_routed_head_sample: Cf=%d + n_class=%d floats do not fit the kernel's LDS", a.Cf, a.n_class);
    return T2H_ERR_UNSUPPORTED;
  }
  const bool trunc = trunc_settings(a.n_class, &a.top_k, &a.top_p_q);
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(T2H_TAIL_KERNEL(routed_head_sample_kernel, ), dim3(a.n), dim3(RS_THREADS), lds, s, a, params,
                     params ? rows_per_sample : 0);
  T2H_CHECK_LAUNCH("t2h_routed_head_sample");
  return T2H_OK;
}

extern "C" int64_t t2h_confidence_group_ws_ints(int32_t n, int32_t n_heads) {
  if (n <= 0 || n_heads <= 0) return 0;
  return (int64_t)CT_HDR + 3 * (int64_t)conf_max_tiles(n, n_heads) + n;
}

// params == NULL: the launch's scalars (t2h_confidence_tail); else the PER_SAMPLE instances (a.temp / a.top_k /
// a.top_p_q are not read)
static int confidence_tail_launch(const t2h_confidence_tail_args* args, const t2h_sample_params* params, int32_t T,
                                  void* stream) {
  T2H_REQUIRE(args != nullptr, "t2h_confidence_tail: args is NULL");
  t2h_confidence_tail_args a = *args;
  if (params) a.temp = 1.f, a.top_k = 0, a.top_p_q = 0;
  T2H_REQUIRE(a.hidden && a.lnf_gamma && a.lnf_beta && a.w_heads && a.tex && a.x_t && a.group_ws && a.logits_ws &&
                  a.tok && a.conf,
              "t2h_confidence_tail: NULL pointer");
  T2H_REQUIRE(a.n > 0 && a.n_class > 0 && a.temp > 0.f && a.n_heads > 0 && a.n_heads <= T2H_MAX_HEADS &&
                  (int64_t)a.n * a.n_class < ((int64_t)1 << 40),
              "t2h_confidence_tail: bad arguments");
  T2H_REQUIRE(a.C == 512, "t2h_confidence_tail: C=%d unsupported (512)", a.C);
  T2H_REQUIRE(a.expo != nullptr || (a.philox_grid_threads != 0 && (a.philox_offset_dev || a.philox_offset % 4 == 0)),
              "t2h_confidence_tail: no noise (expo, or philox_grid_threads and an offset that is a multiple of 4)");
  T2H_TRUNC_REQUIRE("t2h_confidence_tail", a.top_k, a.top_p_q, a.n_class);
  const bool trunc = trunc_settings(a.n_class, &a.top_k, &a.top_p_q);
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(conf_group_kernel, dim3(1), dim3(1024), 0, s, a.x_t, a.tex, a.mask_id, a.n, a.n_heads, a.group_ws);
  const dim3 lgrid(conf_max_tiles(a.n, a.n_heads) * CT_SPLIT), pgrid((a.n + CP_ROWS - 1) / CP_ROWS);
  if (params) T2H_PER_SAMPLE_REQUIRE("t2h_confidence_tail_per_sample", params, T, a.n, a.n_class);
  hipLaunchKernelGGL((params ? conf_logits_kernel<512, true> : conf_logits_kernel<512, false>), lgrid, dim3(CT_THREADS), 0,
                     s, a, params, T);
  hipLaunchKernelGGL(T2H_TAIL_KERNEL(conf_pick_kernel, ), pgrid, dim3(64 * CP_ROWS), 0, s, a, params, T);
  T2H_CHECK_LAUNCH("t2h_confidence_tail");
  return T2H_OK;
}

extern "C" int t2h_confidence_tail(const t2h_confidence_tail_args* args, void* stream) {
  return confidence_tail_launch(args, nullptr, 0, stream);
}

extern "C" int t2h_confidence_tail_per_sample(const t2h_confidence_tail_args* args, const t2h_sample_params* params,
                                              int32_t rows_per_sample, void* stream) {
  T2H_REQUIRE(params != nullptr, "t2h_confidence_tail_per_sample: params is NULL");
  return confidence_tail_launch(args, params, rows_per_sample, stream);
}

template <bool PER_SAMPLE>
static int confidence_commit_launch(const t2h_confidence_commit_args* args, void* stream) {
  T2H_REQUIRE(args != nullptr, "t2h_confidence_commit: args is NULL");
  const t2h_confidence_commit_args a = *args;
  T2H_REQUIRE(a.conf && a.tok && a.tex && a.k && a.tau && a.x_t && a.out, "t2h_confidence_commit: NULL pointer");
  T2H_REQUIRE(a.B > 0 && a.T > 0 && a.T <= CC_MAX_T && a.n_heads > 0 && a.n_heads <= T2H_MAX_HEADS && a.n_class > 0,
              "t2h_confidence_commit: bad arguments (B=%d T=%d)", a.B, a.T);
  T2H_REQUIRE(a.u != nullptr || (a.philox_grid_threads != 0 && (a.philox_offset_dev || a.philox_offset % 4 == 0)),
              "t2h_confidence_commit: no noise (u, or philox_grid_threads and an offset that is a multiple of 4)");
  hipLaunchKernelGGL(conf_commit_kernel<PER_SAMPLE>, dim3(a.B), dim3(CC_THREADS), 0, static_cast<hipStream_t>(stream), a);
  T2H_CHECK_LAUNCH("t2h_confidence_commit");
  return T2H_OK;
}

extern "C" int t2h_confidence_commit(const t2h_confidence_commit_args* args, void* stream) {
  return confidence_commit_launch<false>(args, stream);
}

extern "C" int t2h_confidence_commit_per_sample(const t2h_confidence_commit_args* args, void* stream) {
  return confidence_commit_launch<true>(args, stream);
}

extern "C" int t2h_logp_summary(const float* logp, int32_t B, int32_t T, float* sum, int32_t* count, float* min,
                                void* stream) {
  T2H_REQUIRE(logp && sum && count && min, "t2h_logp_summary: NULL pointer");
  T2H_REQUIRE(B > 0 && T > 0, "t2h_logp_summary: bad arguments (B=%d T=%d)", B, T);
  hipLaunchKernelGGL(logp_summary_kernel, dim3(B), dim3(LS_THREADS), 0, static_cast<hipStream_t>(stream), logp, T, sum,
                     count, min);
  T2H_CHECK_LAUNCH("t2h_logp_summary");
  return T2H_OK;
}

extern "C" int t2h_embed_sum4_f32(const int64_t* idx, const int64_t* segm, const int64_t* tex,
                                  const float* tok_emb, const float* pos_emb, const float* segm_emb,
                                  const float* tex_emb, float* x, int32_t B, int32_t T, int32_t C,
                                  void* stream) {
  T2H_REQUIRE(idx && segm && tex && tok_emb && pos_emb && segm_emb && tex_emb && x,
              "t2h_embed_sum4_f32: NULL pointer");
  T2H_REQUIRE(B > 0 && T > 0 && C > 0 && C % 4 == 0, "t2h_embed_sum4_f32: bad shape");
  hipLaunchKernelGGL(embed_sum4_kernel, dim3(B * T), dim3(128), 0, static_cast<hipStream_t>(stream),
                     idx, segm, tex, tok_emb, pos_emb, segm_emb, tex_emb, x, T, C);
  T2H_CHECK_LAUNCH("t2h_embed_sum4_f32");
  return T2H_OK;
}

extern "C" int t2h_unmask_step(const float* rnd, int32_t t, uint8_t* unmasked, uint8_t* changes,
                               const int64_t* tex, int32_t* head_count, int32_t n, int32_t* changed_rows,
                               int32_t n_heads, void* stream) {
  T2H_REQUIRE(rnd && unmasked && changes && tex && head_count, "t2h_unmask_step: NULL pointer");
  T2H_REQUIRE(t >= 1 && n > 0 && n_heads >= 0, "t2h_unmask_step: t=%d n=%d", t, n);
  const float thresh = 1.0f / (float)t;
  hipLaunchKernelGGL(unmask_step_kernel, dim3((n + 255) / 256), dim3(256), 0,
                     static_cast<hipStream_t>(stream), rnd, thresh, unmasked, changes, tex,
                     head_count, n, changed_rows, n_heads);
  T2H_CHECK_LAUNCH("t2h_unmask_step");
  return T2H_OK;
}

extern "C" int t2h_sample_head(const float* hidden, const float* lnf_gamma, const float* lnf_beta,
                               const float* w_head, const float* expo, const uint8_t* changes,
                               const int64_t* tex, int32_t head, float temp, int64_t* x_t,
                               int64_t* out_idx, int32_t n, int32_t C, int32_t n_class,
                               void* stream) {
  T2H_REQUIRE(hidden && lnf_gamma && lnf_beta && w_head && expo && changes && tex && x_t && out_idx,
              "t2h_sample_head: NULL pointer");
  T2H_REQUIRE(n > 0 && n_class > 0 && temp > 0.f, "t2h_sample_head: bad arguments");
  T2H_REQUIRE(C == 512, "t2h_sample_head: C=%d unsupported (512)", C);
  const size_t lds = (size_t)(n_class + 2 * (SH_THREADS / 64)) * sizeof(float);
  hipLaunchKernelGGL(sample_head_kernel<512>, dim3(n), dim3(SH_THREADS), lds,
                     static_cast<hipStream_t>(stream), hidden, lnf_gamma, lnf_beta, w_head, expo,
                     changes, tex, head, temp, x_t, out_idx, n_class);
  T2H_CHECK_LAUNCH("t2h_sample_head");
  return T2H_OK;
}

// params == NULL: the launch's scalars (t2h_sample_heads); else the PER_SAMPLE instances (a.temp / a.top_k / a.top_p_q
// are not read)
static int sample_heads_launch(const t2h_sample_heads_args* args, const t2h_sample_params* params, int32_t T,
                               void* stream) {
  T2H_REQUIRE(args != nullptr, "t2h_sample_heads: args is NULL");
  t2h_sample_heads_args a = *args;
  if (params) a.temp = 1.f, a.top_k = 0, a.top_p_q = 0;
  T2H_REQUIRE(a.hidden && a.lnf_gamma && a.lnf_beta && a.w_heads && a.rows && a.tex && a.x_t && a.out_idx,
              "t2h_sample_heads: NULL pointer");
  T2H_REQUIRE(a.n > 0 && a.n_class > 0 && a.temp > 0.f && a.n_rows >= 0 && a.n_heads > 0 &&
                  a.n_heads <= T2H_MAX_HEADS,
              "t2h_sample_heads: bad arguments");
  T2H_REQUIRE(a.C == 512, "t2h_sample_heads: C=%d unsupported (512)", a.C);
  T2H_REQUIRE(!a.hidden_compact || a.logits_ws != nullptr, "t2h_sample_heads: compact hidden needs the two-launch form");
  T2H_REQUIRE(a.philox_grid_threads == 0 || a.logits_ws != nullptr,
              "t2h_sample_heads: the in-kernel exponential_ draw needs the two-launch form (logits_ws)");
  T2H_REQUIRE((a.row_philox_offset == nullptr || a.philox_grid_threads != 0) &&
                  ((a.expo_rows == nullptr && a.row_philox_offset == nullptr) || a.logits_ws != nullptr),
              "t2h_sample_heads: per-row noise (row_philox_offset / expo_rows) needs the two-launch form and, for "
              "offsets, philox_grid_threads");
  T2H_REQUIRE(a.philox_seed_img == nullptr ||
                  (a.row_philox_offset != nullptr && a.philox_grid_threads != 0 && a.logits_ws != nullptr),
              "t2h_sample_heads: per-image seeds (philox_seed_img) need row_philox_offset, philox_grid_threads and the "
              "two-launch form (logits_ws)");
  T2H_REQUIRE(a.philox_seed_img == nullptr || (a.img_rows > 0 && a.n % a.img_rows == 0),
              "t2h_sample_heads: per-image seeds need img_rows=%d > 0 dividing n=%d", (int)a.img_rows, (int)a.n);
  T2H_TRUNC_REQUIRE("t2h_sample_heads", a.top_k, a.top_p_q, a.n_class);
  const bool trunc = trunc_settings(a.n_class, &a.top_k, &a.top_p_q);
  if (params) T2H_PER_SAMPLE_REQUIRE("t2h_sample_heads_per_sample", params, T, a.n, a.n_class);
  if (a.n_rows == 0) return T2H_OK;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (a.logits_ws) {  // two launches, SL_SPLIT workgroups per row stream the head weights
    const dim3 lgrid(a.n_rows * SL_SPLIT), pgrid(a.n_rows);
    hipLaunchKernelGGL((params ? sample_logits_kernel<512, true> : sample_logits_kernel<512, false>), lgrid,
                       dim3(SL_THREADS), 0, s, a, a.logits_ws, params, T);
    if (a.philox_seed_img)
      hipLaunchKernelGGL(T2H_TAIL_KERNEL_LOGP(sample_pick_kernel, a.logp, true, ), pgrid, dim3(SH_THREADS), 0, s, a, a.logits_ws, params, T);
    else
      hipLaunchKernelGGL(T2H_TAIL_KERNEL_LOGP(sample_pick_kernel, a.logp, false, ), pgrid, dim3(SH_THREADS), 0, s, a, a.logits_ws, params, T);
    T2H_CHECK_LAUNCH("t2h_sample_heads");
    return T2H_OK;
  }
  const size_t lds = (size_t)(a.n_class + 2 * (SH_THREADS / 64)) * sizeof(float);
  hipLaunchKernelGGL(T2H_TAIL_KERNEL_LOGP(sample_heads_kernel, a.logp, 512, ), dim3(a.n_rows), dim3(SH_THREADS), lds, s, a, params, T);
  T2H_CHECK_LAUNCH("t2h_sample_heads");
  return T2H_OK;
}

extern "C" int t2h_sample_heads(const t2h_sample_heads_args* args, void* stream) {
  return sample_heads_launch(args, nullptr, 0, stream);
}

extern "C" int t2h_sample_heads_per_sample(const t2h_sample_heads_args* args, const t2h_sample_params* params,
                                           int32_t rows_per_sample, void* stream) {
  T2H_REQUIRE(params != nullptr, "t2h_sample_heads_per_sample: params is NULL");
  return sample_heads_launch(args, params, rows_per_sample, stream);
}

// Scoring: launch 1 is the sampling call's (the same instantiation and grid, so the same logits), launch 2 reads the
// token.  The noise and truncation fields of `args` are not read.
static int score_heads_launch(const char* name, const t2h_sample_heads_args* args, const t2h_score_out* score,
                              const t2h_sample_params* params, int32_t T, void* stream) {
  T2H_REQUIRE(args != nullptr && score != nullptr, "%s: args / score is NULL", name);
  t2h_sample_heads_args a = *args;
  if (params) a.temp = 1.f;
  T2H_REQUIRE(a.hidden && a.lnf_gamma && a.lnf_beta && a.w_heads && a.rows && a.tex && a.x_t && a.out_idx,
              "%s: NULL pointer", name);
  T2H_REQUIRE(a.logits_ws != nullptr && a.logp != nullptr && score->targets != nullptr,
              "%s: logits_ws, logp and targets are required (the two-launch form only)", name);
  T2H_REQUIRE(a.n > 0 && a.n_class > 0 && a.temp > 0.f && a.n_rows >= 0 && a.n_heads > 0 && a.n_heads <= T2H_MAX_HEADS,
              "%s: bad arguments", name);
  T2H_REQUIRE(a.C == 512, "%s: C=%d unsupported (512)", name, a.C);
  if (params) T2H_PER_SAMPLE_REQUIRE("t2h_score_heads_per_sample", params, T, a.n, a.n_class);
  if (a.n_rows == 0) return T2H_OK;
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL((params ? sample_logits_kernel<512, true> : sample_logits_kernel<512, false>),
                     dim3(a.n_rows * SL_SPLIT), dim3(SL_THREADS), 0, s, a, a.logits_ws, params, T);
  hipLaunchKernelGGL(score_pick_kernel, dim3(a.n_rows), dim3(SH_THREADS), 0, s, a, a.logits_ws, score->targets,
                     score->rank);
  T2H_CHECK_LAUNCH(name);
  return T2H_OK;
}

extern "C" int t2h_score_heads(const t2h_sample_heads_args* args, const t2h_score_out* score, void* stream) {
  return score_heads_launch("t2h_score_heads", args, score, nullptr, 0, stream);
}

extern "C" int t2h_score_heads_per_sample(const t2h_sample_heads_args* args, const t2h_score_out* score,
                                          const t2h_sample_params* params, int32_t rows_per_sample, void* stream) {
  T2H_REQUIRE(params != nullptr, "t2h_score_heads_per_sample: params is NULL");
  return score_heads_launch("t2h_score_heads_per_sample", args, score, params, rows_per_sample, stream);
}

extern "C" int t2h_q_sample(const int64_t* x0, const float* u, const int64_t* t, int32_t num_timesteps,
                            int64_t mask_id, int64_t* x_t, uint8_t* mask, int32_t B, int32_t T, void* stream) {
  T2H_REQUIRE(x0 && u && t && x_t && mask, "t2h_q_sample: NULL pointer");
  T2H_REQUIRE(B > 0 && T > 0 && num_timesteps > 0, "t2h_q_sample: bad arguments");
  const int n = B * T;
  hipLaunchKernelGGL(q_sample_kernel, dim3((n + 255) / 256), dim3(256), 0, static_cast<hipStream_t>(stream), x0, u,
                     t, (float)num_timesteps, mask_id, x_t, mask, T, n);
  T2H_CHECK_LAUNCH("t2h_q_sample");
  return T2H_OK;
}

extern "C" int t2h_masked_ce_heads(const float* hidden, const float* lnf_gamma, const float* lnf_beta,
                                   const float* w_heads, const int64_t* tex, const uint8_t* mask,
                                   const int64_t* gt_lists, float* ce_rows, float* ce_samples, int32_t B, int32_t T,
                                   int32_t C, int32_t n_class, int32_t n_heads, void* stream) {
  T2H_REQUIRE(hidden && lnf_gamma && lnf_beta && w_heads && tex && mask && gt_lists && ce_rows && ce_samples,
              "t2h_masked_ce_heads: NULL pointer");
  T2H_REQUIRE(B > 0 && T > 0 && n_class > 0 && n_heads > 0, "t2h_masked_ce_heads: bad arguments");
  T2H_REQUIRE(C == 512, "t2h_masked_ce_heads: C=%d unsupported (512)", C);
  const size_t lds = (size_t)(n_class + 2 * (SH_THREADS / 64)) * sizeof(float);
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(masked_ce_kernel<512>, dim3(B * T), dim3(SH_THREADS), lds, s, hidden, lnf_gamma, lnf_beta,
                     w_heads, tex, mask, gt_lists, ce_rows, B * T, n_class, n_heads);
  hipLaunchKernelGGL(segment_sum_kernel, dim3(B), dim3(256), 0, s, ce_rows, ce_samples, T);
  T2H_CHECK_LAUNCH("t2h_masked_ce_heads");
  return T2H_OK;
}

extern "C" int t2h_schedule_advance(const int32_t* rows_tbl, const int64_t* aux64_tbl, const int32_t* aux32_tbl,
                                    int32_t* round_ctr, int32_t* cur_rows, int64_t* cur_aux64, int32_t* cur_aux32,
                                    int32_t maxr, void* stream) {
  T2H_REQUIRE(rows_tbl && round_ctr && cur_rows && maxr > 0 && (!aux64_tbl || cur_aux64) && (!aux32_tbl || cur_aux32),
              "t2h_schedule_advance: bad arguments");
  hipLaunchKernelGGL(schedule_advance_kernel, dim3(1), dim3(256), 0, static_cast<hipStream_t>(stream), rows_tbl,
                     aux64_tbl, aux32_tbl, round_ctr, cur_rows, cur_aux64, cur_aux32, maxr);
  T2H_CHECK_LAUNCH("t2h_schedule_advance");
  return T2H_OK;
}

extern "C" int t2h_philox_uniform_f32(uint64_t seed, uint64_t offset, uint32_t grid_threads, float* out,
                                      int64_t numel, void* stream) {
  T2H_REQUIRE(out && numel > 0 && grid_threads > 0 && offset % 4 == 0, "t2h_philox_uniform_f32: bad arguments");
  hipLaunchKernelGGL(philox_uniform_kernel, dim3((unsigned)((numel + 255) / 256)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), seed, offset, grid_threads, out, numel);
  T2H_CHECK_LAUNCH("t2h_philox_uniform_f32");
  return T2H_OK;
}

// keep == NULL: t2h_unmask_schedule; else the KEEP instance.  `name`: the entry point, for its error texts.
static int unmask_schedule_launch(const char* name, uint64_t seed, uint64_t offset, uint32_t rand_grid_threads,
                                  uint32_t rand_inc, uint32_t expo_inc, const int64_t* tex, const uint8_t* keep, int32_t n,
                                  int32_t steps, int32_t n_heads, int32_t* step_of_row, uint32_t* head_mask,
                                  void* stream) {
  T2H_REQUIRE(tex && step_of_row && head_mask, "%s: NULL pointer", name);
  T2H_REQUIRE(n > 0 && steps >= 1 && steps <= SCHED_MAX_STEPS && n_heads > 0 && n_heads <= T2H_MAX_HEADS &&
                  rand_grid_threads > 0 && offset % 4 == 0 && rand_inc % 4 == 0 && expo_inc % 4 == 0,
              "%s: bad arguments (n=%d steps=%d n_heads=%d)", name, n, steps, n_heads);
  hipLaunchKernelGGL((keep ? unmask_schedule_kernel<true> : unmask_schedule_kernel<false>), dim3(1), dim3(SCHED_THREADS), 0,
                     static_cast<hipStream_t>(stream), seed, offset, rand_grid_threads, rand_inc, expo_inc, tex, keep, n,
                     steps, step_of_row, head_mask);
  T2H_CHECK_LAUNCH(name);
  return T2H_OK;
}

extern "C" int t2h_unmask_schedule(uint64_t seed, uint64_t offset, uint32_t rand_grid_threads, uint32_t rand_inc,
                                   uint32_t expo_inc, const int64_t* tex, int32_t n, int32_t steps, int32_t n_heads,
                                   int32_t* step_of_row, uint32_t* head_mask, void* stream) {
  return unmask_schedule_launch("t2h_unmask_schedule", seed, offset, rand_grid_threads, rand_inc, expo_inc, tex, nullptr,
                                n, steps, n_heads, step_of_row, head_mask, stream);
}

extern "C" int t2h_unmask_schedule_keep(uint64_t seed, uint64_t offset, uint32_t rand_grid_threads, uint32_t rand_inc,
                                        uint32_t expo_inc, const int64_t* tex, const uint8_t* keep, int32_t n,
                                        int32_t steps, int32_t n_heads, int32_t* step_of_row, uint32_t* head_mask,
                                        void* stream) {
  T2H_REQUIRE(keep != nullptr, "t2h_unmask_schedule_keep: NULL pointer");
  return unmask_schedule_launch("t2h_unmask_schedule_keep", seed, offset, rand_grid_threads, rand_inc, expo_inc, tex, keep,
                                n, steps, n_heads, step_of_row, head_mask, stream);
}

extern "C" int t2h_unmask_schedule_batch(const uint64_t* seeds, uint32_t rand_grid_threads, uint32_t rand_inc,
                                         uint32_t expo_inc, const int64_t* tex, const uint8_t* keep, int32_t B, int32_t T,
                                         int32_t steps, int32_t n_heads, int32_t* step_of_row, uint32_t* head_mask,
                                         void* stream) {
  T2H_REQUIRE(seeds && tex && step_of_row && head_mask, "t2h_unmask_schedule_batch: NULL pointer");
  T2H_REQUIRE(B > 0 && T > 0 && (int64_t)B * T <= 0x7fffffff && steps >= 1 && steps <= SCHED_MAX_STEPS && n_heads > 0 &&
                  n_heads <= T2H_MAX_HEADS && rand_grid_threads > 0 && rand_inc % 4 == 0 && expo_inc % 4 == 0,
              "t2h_unmask_schedule_batch: bad arguments (B=%d T=%d steps=%d n_heads=%d)", B, T, steps, n_heads);
  hipLaunchKernelGGL((keep ? unmask_schedule_batch_kernel<true> : unmask_schedule_batch_kernel<false>), dim3(B),
                     dim3(SCHED_THREADS), 0, static_cast<hipStream_t>(stream), seeds, rand_grid_threads, rand_inc, expo_inc,
                     tex, keep, T, steps, step_of_row, head_mask);
  T2H_CHECK_LAUNCH("t2h_unmask_schedule_batch");
  return T2H_OK;
}

extern "C" int t2h_edit_prefill(const int64_t* src_lists, const int64_t* tex, const uint8_t* keep, int64_t mask_id,
                                int64_t* x_t, int64_t* out_lists, uint32_t* err, int32_t n, int32_t n_heads,
                                int32_t n_class, void* stream) {
  T2H_REQUIRE(src_lists && tex && keep && err, "t2h_edit_prefill: NULL pointer");
  T2H_REQUIRE(n > 0 && n_heads > 0 && n_heads <= T2H_MAX_HEADS && n_class > 0, "t2h_edit_prefill: bad arguments");
  hipLaunchKernelGGL(edit_prefill_kernel, dim3((n + 255) / 256), dim3(256), 0, static_cast<hipStream_t>(stream),
                     src_lists, tex, keep, mask_id, x_t, out_lists, err, n, n_heads, n_class);
  T2H_CHECK_LAUNCH("t2h_edit_prefill");
  return T2H_OK;
}

extern "C" int t2h_region_keep(const uint8_t* mask_u8, const float* map_f32, uint64_t label_bits, int32_t mode,
                               int32_t B, int32_t H, int32_t W, int32_t th, int32_t tw, uint8_t* keep, void* stream) {
  T2H_REQUIRE(keep && (mode == 0 ? mask_u8 != nullptr : map_f32 != nullptr), "t2h_region_keep: NULL pointer");
  T2H_REQUIRE(mode >= 0 && mode <= 2 && B > 0 && th > 0 && tw > 0 && H >= th && W >= tw && H % th == 0 &&
                  W % tw == 0,
              "t2h_region_keep: bad arguments (mode=%d H=%d W=%d cells %dx%d)", mode, H, W, th, tw);
  const int n_cells = B * th * tw;
  hipLaunchKernelGGL(region_keep_kernel, dim3((n_cells + RK_CELLS - 1) / RK_CELLS), dim3(64 * RK_CELLS), 0,
                     static_cast<hipStream_t>(stream), mask_u8, map_f32, label_bits, mode, H, W, th, tw, n_cells, keep);
  T2H_CHECK_LAUNCH("t2h_region_keep");
  return T2H_OK;
}

extern "C" int t2h_merge_kept_indices(const int64_t* src_lists, const uint8_t* keep, int64_t* dst_lists, int32_t n,
                                      int32_t n_heads, void* stream) {
  T2H_REQUIRE(src_lists && keep && dst_lists, "t2h_merge_kept_indices: NULL pointer");
  T2H_REQUIRE(n > 0 && n_heads > 0, "t2h_merge_kept_indices: bad arguments");
  const int64_t total = (int64_t)n * n_heads;
  hipLaunchKernelGGL(merge_kept_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), src_lists, keep, dst_lists, n, total);
  T2H_CHECK_LAUNCH("t2h_merge_kept_indices");
  return T2H_OK;
}

static bool fold_count_ok(int K) { return K == 2 || K == 4 || K == 8 || K == 16; }

extern "C" int t2h_fold_keep(const uint8_t* keep, int32_t K, int32_t B, int32_t th, int32_t tw, uint8_t* keep_k,
                             void* stream) {
  T2H_REQUIRE(keep_k, "t2h_fold_keep: NULL pointer");
  T2H_REQUIRE(fold_count_ok(K) && B > 0 && th > 0 && tw > 0 && (int64_t)B * th * tw <= 0x7fffffff / 16,
              "t2h_fold_keep: bad arguments (K=%d B=%d cells %dx%d)", K, B, th, tw);
  const int T = th * tw, n = B * T;
  const int64_t total = (int64_t)K * n;
  hipLaunchKernelGGL(fold_keep_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), keep, K, n, T, tw, keep_k, total);
  T2H_CHECK_LAUNCH("t2h_fold_keep");
  return T2H_OK;
}

extern "C" int t2h_fold_gather(const float* logp_k, const int32_t* rank_k, int32_t K, int32_t B, int32_t th, int32_t tw,
                               float* logp, int32_t* rank, void* stream) {
  T2H_REQUIRE(logp_k && logp && (rank == nullptr || rank_k != nullptr), "t2h_fold_gather: NULL pointer");
  T2H_REQUIRE(fold_count_ok(K) && B > 0 && th > 0 && tw > 0 && (int64_t)B * th * tw <= 0x7fffffff / 16,
              "t2h_fold_gather: bad arguments (K=%d B=%d cells %dx%d)", K, B, th, tw);
  const int T = th * tw, n = B * T;
  hipLaunchKernelGGL(fold_gather_kernel, dim3((n + 255) / 256), dim3(256), 0, static_cast<hipStream_t>(stream), logp_k,
                     rank_k, K, n, T, tw, logp, rank);
  T2H_CHECK_LAUNCH("t2h_fold_gather");
  return T2H_OK;
}

extern "C" int t2h_select_lowest(const float* score, const int32_t* count, int32_t B, int32_t T, uint8_t* keep_out,
                                 int32_t* n_sel, void* stream) {
  T2H_REQUIRE(score && count && keep_out && n_sel, "t2h_select_lowest: NULL pointer");
  T2H_REQUIRE(B > 0 && T > 0, "t2h_select_lowest: bad arguments (B=%d T=%d)", B, T);
  if (T > SEL_MAX_T) {
    t2h_set_error("t2h_select_lowest: T=%d rows per image do not fit the kernel's LDS (at most %d)", T, SEL_MAX_T);
    return T2H_ERR_UNSUPPORTED;
  }
  hipLaunchKernelGGL(select_lowest_kernel, dim3(B), dim3(SEL_THREADS), 0, static_cast<hipStream_t>(stream), score, count,
                     T, keep_out, n_sel);
  T2H_CHECK_LAUNCH("t2h_select_lowest");
  return T2H_OK;
}

extern "C" int t2h_accept_merge(const int64_t* cand_lists, const float* cand_score, const float* sum_cand,
                                const float* sum_cur, int32_t always, int64_t* cur_lists, float* cur_score,
                                float* sum_out, uint8_t* accepted, int32_t B, int32_t T, int32_t n_heads, void* stream) {
  T2H_REQUIRE(cand_lists && cand_score && sum_cand && sum_cur && cur_lists && cur_score && sum_out && accepted,
              "t2h_accept_merge: NULL pointer");
  T2H_REQUIRE(B > 0 && T > 0 && n_heads > 0 && (int64_t)B * T <= 0x7fffffff, "t2h_accept_merge: bad arguments");
  const int64_t total = (int64_t)B * T * n_heads;
  hipLaunchKernelGGL(accept_merge_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), cand_lists, cand_score, sum_cand, sum_cur, always ? 1 : 0, cur_lists,
                     cur_score, sum_out, accepted, B, T, total);
  T2H_CHECK_LAUNCH("t2h_accept_merge");
  return T2H_OK;
}

extern "C" int t2h_philox_exponential_f32(uint64_t seed, uint64_t offset, uint32_t grid_threads, float* out,
                                          int64_t numel, void* stream) {
  T2H_REQUIRE(out && numel > 0 && grid_threads > 0 && offset % 4 == 0, "t2h_philox_exponential_f32: bad arguments");
  hipLaunchKernelGGL(philox_exponential_kernel, dim3((unsigned)((numel + 255) / 256)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), seed, offset, grid_threads, out, numel);
  T2H_CHECK_LAUNCH("t2h_philox_exponential_f32");
  return T2H_OK;
}
