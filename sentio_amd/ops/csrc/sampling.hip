// Per-row temperature / top-k / top-p / seeded sampling for gfx950.
//
//   sample_support : logits [B,V] f32 + per-row (T, top_k, top_p)
//                    -> tau [B] f32 (threshold logit), count [B] i32
//   sample_filtered: the same first phase, then a Gumbel-argmax over the kept
//                    set {v : logit_v >= tau} with noise hashed from
//                    (seed_b, step_b, v) -- never from the row index or B.
//   sample_slots   : sample_filtered over a slot table: row r samples with
//                    the parameters of slot[r], skips free slots, writes the
//                    token into tok[slot] and advances step[slot] in place.
//
// One 1024-thread block per row; nothing is sorted.  tau is found by a radix
// descent (4 levels x 8 bits) on an order-preserving uint32 key of the RAW
// logit (z = logit/T is monotone in the logit for T > 0, so the raw key orders
// the row and tau comes out bit-exact).  Each level builds a 256-bin LDS
// histogram, scans it from the top and descends into the bin where the
// cumulative count crosses top_k (top-k) or the cumulative probability mass
// crosses top_p * M_k (top-p, after top-k, renormalised over the survivors).
//
// Probability mass is accumulated in FIXED POINT: m = exp(z - zmax) * 2^40 as
// a 64-bit integer.  Integer adds are associative, so the histogram is
// independent of thread order (bitwise reproducible runs), a bin's sub-bins
// sum exactly to the bin, and the scan is exactly monotone.  The rounding is
// 2^-41 per token, < 1e-7 of the row's mass at V = 152064 -- below an fp32
// tree reduction.
//
// Contention: a peaked row puts ~all tokens into one level-0 bin.  Every wave
// owns a private histogram copy and every thread run-length-aggregates equal
// consecutive bins in registers, so the hot bin takes one LDS atomic per
// thread and pass instead of one per token.
#include "common.h"
#include "sentio_kernels.h"

typedef unsigned long long u64;

#define SF_THREADS 1024
#define SF_WAVES (SF_THREADS / WAVE)
#define SF_BINS 256
#define SF_MASS_SCALE 1099511627776.0f  // 2^40

struct SfShared {
  u64 hist[SF_WAVES * SF_BINS];  // per-wave private histograms
  u64 tot[SF_BINS];
  u64 red64[SF_WAVES];
  float redf[SF_WAVES];
  float redg[SF_WAVES];
  int redi[SF_WAVES];
  u64 bc64[2];
  int bci;
};

// order-preserving float <-> uint32 (larger float => larger key)
__device__ __forceinline__ unsigned sf_key(float x) {
  unsigned u = __float_as_uint(x);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float sf_unkey(unsigned k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// NaN -> -inf (never selected), -0 -> +0 (one key per compare-equal value)
__device__ __forceinline__ float sf_clean(float x) {
  return (x == x) ? x + 0.0f : -INFINITY;
}

__device__ __forceinline__ u64 sf_mass(float x, float xmax, float invT) {
  return (u64)(expf((x - xmax) * invT) * SF_MASS_SCALE);
}

__device__ __forceinline__ u64 sf_shfl_up(u64 v, int off) {
  unsigned lo = __shfl_up((unsigned)v, off, WAVE);
  unsigned hi = __shfl_up((unsigned)(v >> 32), off, WAVE);
  return ((u64)hi << 32) | lo;
}

// Visit every (cleaned logit, index) of a row once.  Rows start at b*V*4
// bytes, which for odd V is not 16-byte aligned: 16-byte loads over the
// aligned body, scalar loads for the (<= 3 + 3) head and tail elements.
template <class F>
__device__ __forceinline__ void sf_foreach(const float* __restrict__ lb, int V,
                                           F&& f) {
  const int mis = (int)((reinterpret_cast<size_t>(lb) >> 2) & 3);
  const int head = min(V, (4 - mis) & 3);
  const int nvec = (V - head) >> 2;
  const f32x4* vp = reinterpret_cast<const f32x4*>(lb + head);
  // four independent 16-byte loads in flight per thread: with one load per
  // iteration a pass is latency-bound (one block streams a whole row)
  int i = threadIdx.x;
  for (; i + 3 * SF_THREADS < nvec; i += 4 * SF_THREADS) {
    f32x4 q[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) q[u] = vp[i + u * SF_THREADS];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int v = head + 4 * (i + u * SF_THREADS);
      f(sf_clean(q[u].x), v);
      f(sf_clean(q[u].y), v + 1);
      f(sf_clean(q[u].z), v + 2);
      f(sf_clean(q[u].w), v + 3);
    }
  }
  for (; i < nvec; i += SF_THREADS) {
    const f32x4 q = vp[i];
    const int v = head + 4 * i;
    f(sf_clean(q.x), v);
    f(sf_clean(q.y), v + 1);
    f(sf_clean(q.z), v + 2);
    f(sf_clean(q.w), v + 3);
  }
  const int done = head + 4 * nvec;
  const int t = threadIdx.x;
  if (t < head) {
    f(sf_clean(lb[t]), t);
  } else if (t - head < V - done) {
    const int v = done + (t - head);
    f(sf_clean(lb[v]), v);
  }
}

// The same visit through a filter: `allow(x, v)` passes x on or returns
// -inf.  SfAll keeps every token, ScAllowed (constrained decoding) the
// tokens of the row's allowed bitset.
struct SfAll {
  __device__ __forceinline__ float operator()(float x, int) const { return x; }
};

template <class A, class F>
__device__ __forceinline__ void sf_foreach(const float* __restrict__ lb, int V,
                                           const A& allow, F&& g) {
  sf_foreach(lb, V, [&](float x, int v) { g(allow(x, v), v); });
}

__device__ __forceinline__ u64 sf_block_sum64(u64 v, SfShared& sh) {
  const int lane = threadIdx.x & (WAVE - 1), wid = threadIdx.x / WAVE;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    unsigned lo = __shfl_xor((unsigned)v, off, WAVE);
    unsigned hi = __shfl_xor((unsigned)(v >> 32), off, WAVE);
    v += ((u64)hi << 32) | lo;
  }
  if (lane == 0) sh.red64[wid] = v;
  __syncthreads();
  u64 out = 0;
  for (int w = 0; w < SF_WAVES; ++w) out += sh.red64[w];
  __syncthreads();
  return out;
}

// Radix descent.  MASS=false: weights are 1 (count);  MASS=true: weights are
// the fixed-point masses.  Finds the largest key K such that
//   sum of weights over {key >= K}  >=  target,
// i.e. the first value group, from the top, at which the cumulative weight
// reaches the target.  pfrac >= 0 (mass mode, no top-k) sets the target to
// pfrac * (row total) once the level-0 histogram knows the total.
// Returns K; above = weight strictly above K's group.
template <bool MASS, class A = SfAll>
__device__ unsigned sf_descend(const float* __restrict__ lb, int V, float xmax,
                               float invT, u64 target, float pfrac,
                               SfShared& sh, u64& above_out,
                               const A& allow = A()) {
  const int lane = threadIdx.x & (WAVE - 1), wid = threadIdx.x / WAVE;
  u64* myh = sh.hist + wid * SF_BINS;
  unsigned prefix = 0;
  u64 above = 0;
  for (int level = 0; level < 4; ++level) {
    const int shift = 24 - 8 * level;
    for (int i = threadIdx.x; i < SF_WAVES * SF_BINS; i += SF_THREADS)
      sh.hist[i] = 0;
    __syncthreads();
    int cur = 0;
    u64 acc = 0;
    sf_foreach(lb, V, allow, [&](float x, int) {
      const unsigned key = sf_key(x);
      if (level > 0 && ((key ^ prefix) >> (shift + 8)) != 0) return;
      const int bin = (int)((key >> shift) & (SF_BINS - 1));
      const u64 w = MASS ? sf_mass(x, xmax, invT) : 1ull;
      if (bin != cur) {
        if (acc) atomicAdd(&myh[cur], acc);
        cur = bin;
        acc = 0;
      }
      acc += w;
    });
    if (acc) atomicAdd(&myh[cur], acc);
    __syncthreads();
    if (threadIdx.x < SF_BINS) {
      u64 t = 0;
      for (int w = 0; w < SF_WAVES; ++w) t += sh.hist[w * SF_BINS + threadIdx.x];
      sh.tot[threadIdx.x] = t;
    }
    __syncthreads();
    if (wid == 0) {
      // lane owns ranks r = 4*lane .. 4*lane+3 from the top (bin = 255 - r)
      u64 c[4];
      u64 s = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        c[j] = sh.tot[SF_BINS - 1 - (4 * lane + j)];
        s += c[j];
      }
      u64 incl = s;
#pragma unroll
      for (int off = 1; off < WAVE; off <<= 1) {
        const u64 o = sf_shfl_up(incl, off);
        if (lane >= off) incl += o;
      }
      const u64 total =
          ((u64)__shfl((unsigned)(incl >> 32), WAVE - 1, WAVE) << 32) |
          __shfl((unsigned)incl, WAVE - 1, WAVE);
      if (level == 0 && pfrac >= 0.f)
        target = (u64)((double)pfrac * (double)total);
      // integer sums are exact, so the target is always reachable; the clamp
      // only keeps a degenerate row (all-zero mass) inside the histogram
      if (target > above + total) target = above + total;
      if (target < 1) target = 1;
      u64 run = above + (incl - s);
      int found = -1;
      u64 fabove = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const u64 nxt = run + c[j];
        if (found < 0 && c[j] > 0 && nxt >= target) {
          found = 4 * lane + j;
          fabove = run;
        }
        run = nxt;
      }
      const u64 bal = __ballot(found >= 0);
      if (bal == 0) {
        if (lane == 0) { sh.bci = SF_BINS - 1; sh.bc64[0] = above; }
      } else if (lane == __ffsll((long long)bal) - 1) {
        sh.bci = found;
        sh.bc64[0] = fabove;
      }
    }
    __syncthreads();
    prefix |= (unsigned)(SF_BINS - 1 - sh.bci) << shift;
    above = sh.bc64[0];
  }
  above_out = above;
  return prefix;
}

// splitmix64 finaliser: row keys from (seed, step)
__device__ __forceinline__ u64 sf_mix64(u64 z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
// Two keyed multiply-xorshift rounds: with the row index gone, rows differ
// only through (k0, k1), so both keys enter between full-avalanche rounds.
__device__ __forceinline__ unsigned sf_hash(unsigned v, unsigned k0,
                                            unsigned k1) {
  unsigned x = v ^ k0;
  x *= 0x9E3779B1u; x ^= x >> 16;
  x *= 0x85EBCA6Bu; x ^= x >> 13;
  x ^= k1;
  x *= 0xC2B2AE35u; x ^= x >> 16;
  x *= 0x27D4EB2Fu; x ^= x >> 15;
  return x;
}

// What phase 1 leaves for phase 2: the row max, 1/T (1 when greedy), the
// threshold logit and whether the row is greedy.  Block-uniform.
struct SfRow {
  float xmax, invT, tau;
  bool greedy;
};

// Pre-pass and phase 1: row statistics, then the threshold logit tau of the
// kept set {v : logit_v >= tau} after top-k then top-p.  Whole block; every
// thread returns the same SfRow.
template <class A = SfAll>
__device__ __forceinline__ SfRow sf_threshold(const float* __restrict__ lb,
                                              int V, float T, int k, float p,
                                              SfShared& sh,
                                              const A& allow = A()) {
  const int lane = threadIdx.x & (WAVE - 1), wid = threadIdx.x / WAVE;
  // ---- pre-pass: row max, smallest finite logit, number of finite logits
  float xmax = -INFINITY, xmin = INFINITY;
  int nfin = 0;
  sf_foreach(lb, V, allow, [&](float x, int) {
    xmax = fmaxf(xmax, x);
    if (x > -INFINITY) { xmin = fminf(xmin, x); ++nfin; }
  });
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    xmax = fmaxf(xmax, __shfl_xor(xmax, off, WAVE));
    xmin = fminf(xmin, __shfl_xor(xmin, off, WAVE));
    nfin += __shfl_xor(nfin, off, WAVE);
  }
  if (lane == 0) { sh.redf[wid] = xmax; sh.redg[wid] = xmin; sh.redi[wid] = nfin; }
  __syncthreads();
  xmax = -INFINITY; xmin = INFINITY; nfin = 0;
  for (int w = 0; w < SF_WAVES; ++w) {
    xmax = fmaxf(xmax, sh.redf[w]);
    xmin = fminf(xmin, sh.redg[w]);
    nfin += sh.redi[w];
  }
  __syncthreads();

  // ---- phase 1: threshold logit
  const bool greedy = !(T > 0.f) || xmax == INFINITY || xmax == -INFINITY;
  const float invT = greedy ? 1.f : 1.f / T;
  float tau;
  if (greedy) {
    tau = xmax;
  } else {
    const bool k_on = k >= 1 && k < nfin;
    const bool p_on = p < 1.f;
    tau = xmin;  // both filters off: every finite logit
    u64 target = 0;
    if (k_on) {
      u64 cgt;
      const unsigned key_k = sf_descend<false>(lb, V, xmax, invT, (u64)k, -1.f,
                                               sh, cgt, allow);
      tau = sf_unkey(key_k);
      if (p_on) {
        // M_k: mass of exactly the k best (ties at the k-th value weigh the
        // same, so which of them count is immaterial)
        u64 part = 0;
        sf_foreach(lb, V, allow, [&](float x, int) {
          if (sf_key(x) > key_k) part += sf_mass(x, xmax, invT);
        });
        const u64 mk = sf_block_sum64(part, sh) +
                       ((u64)k - cgt) * sf_mass(tau, xmax, invT);
        target = (u64)((double)fmaxf(p, 0.f) * (double)mk);
      }
    }
    if (p_on) {
      u64 unused;
      const unsigned key_p = sf_descend<true>(
          lb, V, xmax, invT, target, k_on ? -1.f : fmaxf(p, 0.f), sh, unused,
          allow);
      tau = sf_unkey(key_p);
    }
  }
  return SfRow{xmax, invT, tau, greedy};
}

// Phase 2: Gumbel-argmax over the kept set (plain argmax when greedy), noise
// hashed from (seed, step, v).  Whole block; the token is valid on thread 0
// only, and nothing follows the function's one block barrier but thread 0's
// scan of the per-wave winners.
template <class A = SfAll>
__device__ __forceinline__ long sf_gumbel_argmax(const float* __restrict__ lb,
                                                 int V, const SfRow& r,
                                                 long seed, int step,
                                                 SfShared& sh,
                                                 const A& allow = A()) {
  const int lane = threadIdx.x & (WAVE - 1), wid = threadIdx.x / WAVE;
  const float xmax = r.xmax, invT = r.invT, tau = r.tau;
  const bool greedy = r.greedy;
  const u64 rk = sf_mix64((u64)seed ^
                          sf_mix64((u64)(unsigned)step + 0x9E3779B97F4A7C15ull));
  const unsigned k0 = (unsigned)rk, k1 = (unsigned)(rk >> 32);
  float best = -INFINITY;
  int besti = 0x7fffffff;
  sf_foreach(lb, V, allow, [&](float x, int v) {
    if (!(x >= tau)) return;
    float sc = x;
    if (!greedy) {
      const unsigned h = sf_hash((unsigned)v, k0, k1);
      // u = (2n+1) * 2^-24 with n = top 23 bits: every value is exact in
      // fp32 and lies in [2^-24, 1 - 2^-24].  (A 24-bit n plus 0.5f is NOT
      // representable above 2^23 and rounds up to u == 1, whose Gumbel
      // noise is +inf: that token would win whatever its logit.)
      const float u = (float)(h >> 9) * (1.0f / 8388608.0f)
                      + (1.0f / 16777216.0f);
      // -log(u) >= 2^-24 for every such u; the clamp keeps the fast log's
      // rounding near u = 1 from ever reaching 0
      const float e = fmaxf(-__logf(u), 5.9604645e-8f);
      sc = (x - xmax) * invT - __logf(e);
    }
    if (sc > best || (sc == best && v < besti)) { best = sc; besti = v; }
  });
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const float ov = __shfl_xor(best, off, WAVE);
    const int oi = __shfl_xor(besti, off, WAVE);
    if (ov > best || (ov == best && oi < besti)) { best = ov; besti = oi; }
  }
  if (lane == 0) { sh.redf[wid] = best; sh.redi[wid] = besti; }
  __syncthreads();
  int bi = 0;
  if (threadIdx.x == 0) {
    float bv = sh.redf[0];
    bi = sh.redi[0];
    for (int w = 1; w < SF_WAVES; ++w)
      if (sh.redf[w] > bv || (sh.redf[w] == bv && sh.redi[w] < bi)) {
        bv = sh.redf[w];
        bi = sh.redi[w];
      }
  }
  return (bi < V) ? bi : 0;
}

template <bool SAMPLE>
__global__ __launch_bounds__(SF_THREADS) void sample_filtered_kernel(
    const float* __restrict__ logits, const float* __restrict__ temperature,
    const int* __restrict__ top_k, const float* __restrict__ top_p,
    const long* __restrict__ seed, const int* __restrict__ step,
    float* __restrict__ tau_out, int* __restrict__ count_out,
    long* __restrict__ tok_out, int V) {
  __shared__ SfShared sh;
  const long b = blockIdx.x;
  const float* lb = logits + b * (long)V;
  const SfRow r = sf_threshold(lb, V, temperature[b], top_k[b], top_p[b], sh);

  if (!SAMPLE) {
    const int lane = threadIdx.x & (WAVE - 1), wid = threadIdx.x / WAVE;
    const float tau = r.tau;
    int cnt = 0;
    sf_foreach(lb, V, [&](float x, int) { cnt += (x >= tau) ? 1 : 0; });
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off, WAVE);
    if (lane == 0) sh.redi[wid] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
      int c = 0;
      for (int w = 0; w < SF_WAVES; ++w) c += sh.redi[w];
      tau_out[b] = tau;
      count_out[b] = c;
    }
    return;
  }

  const long tok = sf_gumbel_argmax(lb, V, r, seed[b], step[b], sh);
  if (threadIdx.x == 0) tok_out[b] = tok;
}

// The slot loop's sampler: logits row r belongs to slot s = slot ? slot[r] : r
// of S persistent slots, each with its own (T, top_k, top_p, seed) and a step
// counter that lives on the device.  A row whose slot is outside [0, S) or
// whose slot is inactive returns before any barrier or store (s is
// block-uniform).  Otherwise: sample_filtered's arithmetic at step[s], token
// to tok[s], step[s] + 1 to step[s].  Two rows on one slot would race on
// step[s]: callers pass each slot at most once.
__global__ __launch_bounds__(SF_THREADS) void sample_slots_kernel(
    const float* __restrict__ logits, const int* __restrict__ slot,
    const float* __restrict__ temperature, const int* __restrict__ top_k,
    const float* __restrict__ top_p, const long* __restrict__ seed,
    int* __restrict__ step, const unsigned char* __restrict__ active,
    long* __restrict__ tok, int S, int V) {
  __shared__ SfShared sh;
  const long row = blockIdx.x;
  const int s = slot ? slot[row] : (int)row;
  if (s < 0 || s >= S) return;
  if (active && active[s] == 0) return;
  const int st = step[s];
  const float* lb = logits + row * (long)V;
  const SfRow r = sf_threshold(lb, V, temperature[s], top_k[s], top_p[s], sh);
  const long t = sf_gumbel_argmax(lb, V, r, seed[s], st, sh);
  if (threadIdx.x == 0) {
    tok[s] = t;
    step[s] = st + 1;
  }
}

// ---- grammar-constrained sampling
//
// A row in automaton state s (0 <= s < N) with `left` tokens remaining may
// pick token v iff v < Vc = min(V, Vt), bit v of mask[s] is set and
// dist[next[s, v]] <= left - 1.  The allowed set is built ONCE per row as a
// bitset in LDS: every mask word is loaded once (one word per 32 tokens),
// and only when the budget can bind (left - 1 < max_dist, block-uniform)
// does a second sweep read next[s, .] (one contiguous int16 row) and dist
// through it to clear tokens that could no longer finish in time.  The
// passes of sf_threshold / sf_gumbel_argmax then see -inf for every other
// token and read only the first Vc logits of the row.
#define SC_MAX_WORDS 2048  // bitset words in LDS: Vt <= 65536

struct ScAllowed {
  const unsigned* bits;
  __device__ __forceinline__ float operator()(float x, int v) const {
    return ((bits[v >> 5] >> (v & 31)) & 1u) ? x : -INFINITY;
  }
};

// Whole block.  s is a valid state; ends on a block barrier.
__device__ __forceinline__ void sc_build_allowed(
    unsigned* bits, const int* __restrict__ mask,
    const short* __restrict__ next, const short* __restrict__ dist, int s,
    int left, int Vc, int Vt, int N, int W, int max_dist) {
  const int nw = (Vc + 31) >> 5;
  for (int w = threadIdx.x; w < nw; w += SF_THREADS) {
    unsigned m = (unsigned)mask[(long)s * W + w];
    const int rem = Vc - 32 * w;  // >= 1
    if (rem < 32) m &= (1u << rem) - 1u;
    bits[w] = m;
  }
  __syncthreads();
  if (left - 1 < max_dist) {
    const short* nr = next + (long)s * Vt;
    for (int v = threadIdx.x; v < Vc; v += SF_THREADS) {
      const unsigned bit = 1u << (v & 31);
      if (bits[v >> 5] & bit) {
        const int nx = nr[v];
        const bool ok = nx >= 0 && nx < N && (int)dist[nx] <= left - 1;
        if (!ok) atomicAnd(&bits[v >> 5], ~bit);
      }
    }
    __syncthreads();
  }
}

// Thread 0, after the last barrier: the token of a constrained row.  A row
// whose allowed logits are all -inf / NaN takes the lowest allowed index
// (the unconstrained fallthrough, token 0, is PAD).  Returns -1 when
// nothing is allowed at all.
__device__ __forceinline__ long sc_finish(const unsigned* bits, int Vc,
                                          const SfRow& r, long tok) {
  if (r.xmax == -INFINITY) {
    tok = -1;
    const int nw = (Vc + 31) >> 5;
    for (int w = 0; w < nw; ++w)
      if (bits[w]) { tok = 32 * w + __ffs((int)bits[w]) - 1; break; }
  }
  return tok;
}

// SLOTS=false: row b samples with (temperature, top_k, top_p, seed, step,
// state, left)[b] and writes tok[b].  SLOTS=true: sample_slots_kernel's
// addressing (slot / active, arrays are [S], step advanced).  A row whose
// state is outside [0, N) is unconstrained: sample_filtered's arithmetic
// over all V logits, state and left untouched.  Otherwise state[i] =
// next[state, tok] and left[i] -= 1.  Every early return is block-uniform.
template <bool SLOTS>
__global__ __launch_bounds__(SF_THREADS) void sample_constrained_kernel(
    const float* __restrict__ logits, const int* __restrict__ slot,
    const float* __restrict__ temperature, const int* __restrict__ top_k,
    const float* __restrict__ top_p, const long* __restrict__ seed,
    int* __restrict__ step, const unsigned char* __restrict__ active,
    long* __restrict__ tok, int* __restrict__ state, int* __restrict__ left,
    const short* __restrict__ next, const int* __restrict__ mask,
    const short* __restrict__ dist, int S, int V, int Vt, int N, int W,
    int max_dist) {
  __shared__ SfShared sh;
  __shared__ unsigned bits[SC_MAX_WORDS];
  const long row = blockIdx.x;
  int s = (int)row;
  if (SLOTS) {
    s = slot ? slot[row] : (int)row;
    if (s < 0 || s >= S) return;
    if (active && active[s] == 0) return;
  }
  const int st = step[s];
  const int q = state[s];
  const float* lb = logits + row * (long)V;
  const float T = temperature[s];
  const int k = top_k[s];
  const float p = top_p[s];
  const long sd = seed[s];
  if (q < 0 || q >= N) {
    const SfRow r = sf_threshold(lb, V, T, k, p, sh);
    const long t = sf_gumbel_argmax(lb, V, r, sd, st, sh);
    if (threadIdx.x == 0) {
      tok[s] = t;
      if (SLOTS) step[s] = st + 1;
    }
    return;
  }
  const int lf = left[s];
  const int Vc = min(V, Vt);
  sc_build_allowed(bits, mask, next, dist, q, lf, Vc, Vt, N, W, max_dist);
  const ScAllowed allow{bits};
  const SfRow r = sf_threshold(lb, Vc, T, k, p, sh, allow);
  long t = sf_gumbel_argmax(lb, Vc, r, sd, st, sh, allow);
  if (threadIdx.x == 0) {
    t = sc_finish(bits, Vc, r, t);
    // nothing allowed (a budget the caller did not establish): PAD, and the
    // row keeps its state
    const bool ok = t >= 0 && t < Vc && ((bits[t >> 5] >> (t & 31)) & 1u);
    tok[s] = ok ? t : 0;
    if (ok) {
      state[s] = next[(long)q * Vt + t];
      left[s] = lf - 1;
    }
    if (SLOTS) step[s] = st + 1;
  }
}

extern "C" {

static bool sc_tables_ok(int V, int Vt, int N, int W, int max_dist) {
  return V > 0 && Vt > 0 && N >= 1 && N <= 32767 && W == (Vt + 31) / 32 &&
         W <= SC_MAX_WORDS && max_dist >= 0;
}

hipError_t sentio_sample_constrained(
    const float* logits, const float* temperature, const int* top_k,
    const float* top_p, const long* seed, const int* step, int* state,
    int* left, const short* next, const int* mask, const short* dist,
    long* tok, long B, int V, int Vt, int N, int W, int max_dist,
    hipStream_t stream) {
  if (B <= 0 || B > 0x7fffffffL || !sc_tables_ok(V, Vt, N, W, max_dist))
    return hipErrorInvalidValue;
  // SLOTS=false never writes step
  hipLaunchKernelGGL((sample_constrained_kernel<false>), dim3((unsigned)B),
                     dim3(SF_THREADS), 0, stream, logits, (const int*)nullptr,
                     temperature, top_k, top_p, seed, const_cast<int*>(step),
                     (const unsigned char*)nullptr, tok, state, left, next,
                     mask, dist, (int)B, V, Vt, N, W, max_dist);
  HIP_CHECK_LAUNCH();
  return hipSuccess;
}

hipError_t sentio_sample_slots_constrained(
    const float* logits, const int* slot, const float* temperature,
    const int* top_k, const float* top_p, const long* seed, int* step,
    const unsigned char* active, long* tok, int* state, int* left,
    const short* next, const int* mask, const short* dist, long R, int S,
    int V, int Vt, int N, int W, int max_dist, hipStream_t stream) {
  if (R <= 0 || S <= 0 || R > 0x7fffffffL ||
      !sc_tables_ok(V, Vt, N, W, max_dist))
    return hipErrorInvalidValue;
  if (!slot && R != S) return hipErrorInvalidValue;
  hipLaunchKernelGGL((sample_constrained_kernel<true>), dim3((unsigned)R),
                     dim3(SF_THREADS), 0, stream, logits, slot, temperature,
                     top_k, top_p, seed, step, active, tok, state, left, next,
                     mask, dist, S, V, Vt, N, W, max_dist);
  HIP_CHECK_LAUNCH();
  return hipSuccess;
}

hipError_t sentio_sample_support(const float* logits, const float* temperature,
                                 const int* top_k, const float* top_p,
                                 float* tau, int* count, long B, int V,
                                 hipStream_t stream) {
  if (B <= 0 || V <= 0 || B > 0x7fffffffL) return hipErrorInvalidValue;
  hipLaunchKernelGGL((sample_filtered_kernel<false>), dim3((unsigned)B),
                     dim3(SF_THREADS), 0, stream, logits, temperature, top_k,
                     top_p, (const long*)nullptr, (const int*)nullptr, tau,
                     count, (long*)nullptr, V);
  HIP_CHECK_LAUNCH();
  return hipSuccess;
}

hipError_t sentio_sample_filtered(const float* logits, const float* temperature,
                                  const int* top_k, const float* top_p,
                                  const long* seed, const int* step, long* out,
                                  long B, int V, hipStream_t stream) {
  if (B <= 0 || V <= 0 || B > 0x7fffffffL) return hipErrorInvalidValue;
  hipLaunchKernelGGL((sample_filtered_kernel<true>), dim3((unsigned)B),
                     dim3(SF_THREADS), 0, stream, logits, temperature, top_k,
                     top_p, seed, step, (float*)nullptr, (int*)nullptr, out, V);
  HIP_CHECK_LAUNCH();
  return hipSuccess;
}

hipError_t sentio_sample_slots(const float* logits, const int* slot,
                               const float* temperature, const int* top_k,
                               const float* top_p, const long* seed, int* step,
                               const unsigned char* active, long* tok, long R,
                               int S, int V, hipStream_t stream) {
  if (R <= 0 || S <= 0 || V <= 0 || R > 0x7fffffffL) return hipErrorInvalidValue;
  // without a slot table row r is slot r: every row needs a slot of its own
  if (!slot && R != S) return hipErrorInvalidValue;
  hipLaunchKernelGGL(sample_slots_kernel, dim3((unsigned)R), dim3(SF_THREADS),
                     0, stream, logits, slot, temperature, top_k, top_p, seed,
                     step, active, tok, S, V);
  HIP_CHECK_LAUNCH();
  return hipSuccess;
}

}  // extern "C"
