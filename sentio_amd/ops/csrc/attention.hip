// Attention kernels for gfx950 (CDNA4):
//  * flash_attn  — prefill: flash-style online-softmax attention on
//    mfma_f32_16x16x32_bf16, never materializing the S×S score matrix.
//    One wave per (batch, head, 16-row Q tile); K staged XOR-swizzled in LDS
//    (row-major D-stride tiles are an up-to-16-way bank conflict — guide §6
//    G4), V staged transposed so the PV B-fragment is a contiguous
//    ds_read_b128, P round-trips through padded LDS for the C→A relayout.
//  * decode_attn — single-token decode, split-S ("flash-decoding"): one
//    block per (kv-head, batch, split) streams its key range of the
//    contiguous KV cache once for all G query heads of the group with a
//    chunked online softmax; a combine kernel reduces the splits.
//
// Replaces (K6 prefill/decode in SURVEY §2.3) the reference's remote
// /chat/completions calls (reference src/core/llm/providers/openai.py:117).
#include "common.h"
#include "sentio_kernels.h"

typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
typedef float f32x4_t __attribute__((ext_vector_type(4)));

// MFMA fragment maps for mfma_f32_16x16x32_bf16 (guide §3):
//   A[16m x 32k]: lane l -> row = l&15,  k = (l>>4)*8 + j   (j = 0..7)
//   B[32k x 16n]: lane l -> col = l&15,  k = (l>>4)*8 + j
//   C/D[16m x 16n]: lane l, reg r -> col = l&15, row = (l>>4)*4 + r

#define QBLK 16
#define KVBLK 64   // keys per staged tile: amortizes softmax/barrier/staging
#define MAXD 128

// LDS byte-offset helpers
// K tile [KVBLK][D] bf16, XOR-swizzled: byte ^= (row&7)<<4
__device__ __forceinline__ int k_lds_off(int row, int d_byte, int Dbytes) {
  return (row * Dbytes + d_byte) ^ ((row & 7) << 4);
}
// V tile image for ds_read_b64_tr_b16 (gfx950 hardware transpose-read,
// guide §LDS): per 16-dim block db, 8 slots of 4(key)x16(dim) bf16 tiles,
// evens-then-odds slot order so a wave's 16-lane group g finds its PV
// fragment's keys 8g+0..3 at slot g and keys 8g+4..7 at slot g+4 — the
// second read is one uniform +512 B offset.  Staging stays vectorized
// 16 B row-major writes (the old V^T image needed 8 scalar stores per
// load); the fragment read is 2 tr-reads instead of 8 scalar ds_reads.
typedef __bf16 bf16x4_t __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) bf16x4_t* lds_v4_ptr;
#define V_SLOTS (KVBLK / 4)
__device__ __forceinline__ int v_tr_off(int key, int d) {  // element offset
  const int db = d >> 4, kb = key >> 2;
  const int slot = (kb & 1) ? (KVBLK / 8) + (kb >> 1) : (kb >> 1);
  return (db * V_SLOTS + slot) * 64 + (key & 3) * 16 + (d & 15);
}
// P tile [QBLK][KVBLK] bf16 with 16-byte row pad
#define P_STRIDE (KVBLK * 2 + 16)

// 4 waves per block: waves handle 4 consecutive 16-row Q tiles of ONE
// (batch, head) and SHARE the K/V LDS staging — 4x less HBM/LDS staging
// traffic than wave-private tiles, cooperative 256-thread staging.
// (Measured r2: FA_WAVES=8 with correctly sized LDS is 3-4% SLOWER —
// 153 vs 159 TF/s — and KVBLK=128 much slower, 94 TF/s: bigger shared
// tiles cost occupancy/barrier latency more than they save staging.)
#define FA_WAVES 4

// QT q-tiles (16 rows each) per wave: the K fragment loads and the V
// transpose-reads are shared across the wave's QT row-tiles, and every
// barrier/staging pass serves QT x 16 rows — per-row overhead halves at
// QT=2 vs the one-tile version.
#define FA_QT 1   // measured: QT=2 amortizes fragments but costs occupancy (124 vs 156 TF/s) — QT=1 wins
// CACHE_SRC=false: K/V are activation tensors [B, S, Hkv, D] (plain
// prefill).  CACHE_SRC=true: K/V are KV-cache tensors [B, Hkv, Smax, D]
// and the queries are a SUFFIX starting at absolute position q_off —
// prefix-KV-cached prefill attends to cache rows [0, kv_lens[b]).
template <int DT, bool CACHE_SRC>
__launch_bounds__(FA_WAVES * WAVE)
__global__ void flash_attn_kernel(
    const bf16* __restrict__ q,    // [B, S, H, D] (S = suffix len if CACHE_SRC)
    const bf16* __restrict__ k,
    const bf16* __restrict__ v,
    bf16* __restrict__ out,        // [B, S, H, D]
    const int* __restrict__ kv_lens,  // [B] (absolute KV lengths)
    int B, int S, int H, int Hkv, int D_, float scale, int causal,
    int Smax, int q_off) {
  constexpr int D = DT;            // compile-time: every staging/frag loop
                                   // unrolls, loads batch before waits
  constexpr int QT = FA_QT;
  constexpr int WROWS = QT * QBLK; // q rows per wave
  extern __shared__ __attribute__((aligned(16))) char smem[];
  // carve: K tile | V tr image | per-wave P tiles
  char* k_lds = smem;                                   // KVBLK * D * 2
  char* vt_lds = k_lds + KVBLK * D * 2;                 // KVBLK * D * 2

  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x / WAVE;
  char* p_lds = vt_lds + KVBLK * D * 2 + wid * WROWS * P_STRIDE;

  const int h = blockIdx.y;
  const int b = blockIdx.z;
  const int hkv = h / (H / Hkv);
  const int q0 = (blockIdx.x * FA_WAVES + wid) * WROWS;
  const int kvlen = CACHE_SRC ? min(kv_lens[b], Smax) : min(kv_lens[b], S);
  const bool active = q0 < S;           // inactive waves still hit barriers

  constexpr int DC = D / 32;            // feature chunks per mfma K-dim
  constexpr int NB = D / 16;            // output column blocks

  // ---- load Q fragments per tile t:
  // a_q[t][dc] = Q[q0 + t*16 + (l&15)][dc*32 + (l>>4)*8 + j]
  const int arow = lane & 15;
  const int kofs = (lane >> 4) * 8;
  bf16x8_t a_q[QT][DC];
#pragma unroll
  for (int t = 0; t < QT; ++t) {
    const int qrow = q0 + t * QBLK + arow;
    const bf16* qp = q + (((long)b * S + qrow) * H + h) * D + kofs;
#pragma unroll
    for (int dc = 0; dc < DC; ++dc) {
      if (qrow < S) {
        a_q[t][dc] = *reinterpret_cast<const bf16x8_t*>(qp + dc * 32);
      } else {
        bf16x8_t z = {};
        a_q[t][dc] = z;
      }
    }
  }

  // ---- accumulators (per tile)
  f32x4_t o_acc[QT][NB];
  float m_run[QT][4], l_run[QT][4];
#pragma unroll
  for (int t = 0; t < QT; ++t) {
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) o_acc[t][nb] = f32x4_t{};
#pragma unroll
    for (int r = 0; r < 4; ++r) { m_run[t][r] = -INFINITY; l_run[t][r] = 0.f; }
  }

  // block-level kv bound: the LAST wave's causal horizon
  const int block_q_hi = min(blockIdx.x * FA_WAVES * WROWS + FA_WAVES * WROWS,
                             S);
  const int kv_hi = causal ? min(kvlen, q_off + block_q_hi) : kvlen;
  const int n_kv_tiles = (kv_hi + KVBLK - 1) / KVBLK;

  // T14 software-pipelined staging (guide §6: attention staging →
  // register staging, split): tile kt's K/V live in registers while tile
  // kt-1 computes; the loads for kt+1 issue right after the stores of kt
  // land, so HBM latency hides under QK/softmax/PV of the previous tile.
  constexpr int ST_ELEMS = KVBLK * D;
  constexpr int ST_STRIDE = FA_WAVES * WAVE * 8;
  constexpr int ST_IT = (ST_ELEMS + ST_STRIDE - 1) / ST_STRIDE;
  bf16x8_t kvals[ST_IT], vvals[ST_IT];

  auto load_tile = [&](int kt) {
    const int kv0 = kt * KVBLK;
#pragma unroll
    for (int u = 0; u < ST_IT; ++u) {
      const int i = threadIdx.x * 8 + u * ST_STRIDE;
      const int key = kv0 + i / D;
      const int d = i % D;
      if (i < ST_ELEMS && key < kvlen) {
        const long base = CACHE_SRC
            ? (((long)b * Hkv + hkv) * Smax + key) * D + d
            : (((long)b * S + key) * Hkv + hkv) * D + d;
        kvals[u] = *reinterpret_cast<const bf16x8_t*>(k + base);
        vvals[u] = *reinterpret_cast<const bf16x8_t*>(v + base);
      } else {
        bf16x8_t z = {};
        kvals[u] = z;
        vvals[u] = z;
      }
    }
  };
  auto store_tile = [&]() {
#pragma unroll
    for (int u = 0; u < ST_IT; ++u) {
      const int i = threadIdx.x * 8 + u * ST_STRIDE;
      if (i < ST_ELEMS) {
        const int row = i / D, d = i % D;
        *reinterpret_cast<bf16x8_t*>(k_lds + k_lds_off(row, d * 2, D * 2)) =
            kvals[u];
        *reinterpret_cast<bf16x8_t*>(vt_lds + v_tr_off(row, d) * 2) = vvals[u];
      }
    }
  };

  if (n_kv_tiles > 0) load_tile(0);
  for (int kt = 0; kt < n_kv_tiles; ++kt) {
    const int kv0 = kt * KVBLK;
    store_tile();
    __syncthreads();  // staging visible to every wave
    if (kt + 1 < n_kv_tiles) load_tile(kt + 1);  // in flight under compute

    // waves whose causal horizon ends before this kv tile skip compute but
    // still execute every barrier (uniform control flow)
    const int wave_q_hi = min(q0 + WROWS - 1, S - 1);
    const bool compute = active && (!causal || kv0 <= q_off + wave_q_hi);

    constexpr int HALVES = KVBLK / 16;
    float alpha[QT][4];
    if (compute) {
      // ---- S = scale * Q K^T: K B-frag loaded ONCE per (half, dc),
      // reused by every q tile
      f32x4_t s_acc[QT][HALVES];
#pragma unroll
      for (int t = 0; t < QT; ++t)
#pragma unroll
        for (int half = 0; half < HALVES; ++half) s_acc[t][half] = f32x4_t{};
#pragma unroll
      for (int half = 0; half < HALVES; ++half) {
#pragma unroll
        for (int dc = 0; dc < DC; ++dc) {
          const int krow = half * 16 + (lane & 15);
          bf16x8_t b_frag = *reinterpret_cast<const bf16x8_t*>(
              k_lds + k_lds_off(krow, (dc * 32 + kofs) * 2, D * 2));
#pragma unroll
          for (int t = 0; t < QT; ++t)
            s_acc[t][half] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                a_q[t][dc], b_frag, s_acc[t][half], 0, 0, 0);
        }
      }

      // ---- online softmax per tile; P written to the wave's LDS buffer
#pragma unroll
      for (int t = 0; t < QT; ++t) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int qrow_local = (lane >> 4) * 4 + r;
          const int qrow = q0 + t * QBLK + qrow_local;
          float sv[HALVES];
          float rmax_l = -INFINITY;
#pragma unroll
          for (int half = 0; half < HALVES; ++half) {
            const int key = kv0 + half * 16 + (lane & 15);
            const bool ok = key < kvlen && (!causal || key <= q_off + qrow);
            sv[half] = ok ? s_acc[t][half][r] * scale : -INFINITY;
            rmax_l = fmaxf(rmax_l, sv[half]);
          }
          float rmax = group16_max(rmax_l);
          float m_new = fmaxf(m_run[t][r], rmax);
          float a = (m_run[t][r] == -INFINITY) ? 0.f
                    : __expf(m_run[t][r] - m_new);
          if (m_new == -INFINITY) a = 1.f;  // nothing seen yet at all
          alpha[t][r] = a;
          float psum = 0.f;
#pragma unroll
          for (int half = 0; half < HALVES; ++half) {
            const float pv = (sv[half] == -INFINITY)
                                 ? 0.f : __expf(sv[half] - m_new);
            psum += pv;
            *reinterpret_cast<__bf16*>(
                p_lds + (t * QBLK + qrow_local) * P_STRIDE +
                (half * 16 + (lane & 15)) * 2) = (__bf16)pv;
          }
          float rsum = group16_sum(psum);
          l_run[t][r] = l_run[t][r] * a + rsum;
          m_run[t][r] = m_new;
        }
      }
    }
    __syncthreads();
    if (compute) {
      // A frags for PV per tile and 32-key chunk
      bf16x8_t a_p[QT][KVBLK / 32];
#pragma unroll
      for (int t = 0; t < QT; ++t)
#pragma unroll
        for (int kc = 0; kc < KVBLK / 32; ++kc)
          a_p[t][kc] = *reinterpret_cast<const bf16x8_t*>(
              p_lds + (t * QBLK + (lane & 15)) * P_STRIDE +
              (kc * 32 + kofs) * 2);

      // ---- O = alpha*O + P V: V tr-reads loaded once per (nb, kc),
      // reused by every q tile
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) {
#pragma unroll
        for (int t = 0; t < QT; ++t)
#pragma unroll
          for (int r = 0; r < 4; ++r) o_acc[t][nb][r] *= alpha[t][r];
        char* vb_base = vt_lds + nb * (V_SLOTS * 128) + (long)lane * 8;
#pragma unroll
        for (int kc = 0; kc < KVBLK / 32; ++kc) {
          bf16x4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
              (lds_v4_ptr)(vb_base + kc * 512));
          bf16x4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
              (lds_v4_ptr)(vb_base + kc * 512 + (KVBLK / 8) * 128));
          bf16x8_t b_v;
#pragma unroll
          for (int j = 0; j < 4; ++j) { b_v[j] = lo[j]; b_v[4 + j] = hi[j]; }
#pragma unroll
          for (int t = 0; t < QT; ++t)
            o_acc[t][nb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                a_p[t][kc], b_v, o_acc[t][nb], 0, 0, 0);
        }
      }
    }
    __syncthreads();
  }

  // ---- epilogue: divide by l, store
  if (!active) return;
#pragma unroll
  for (int t = 0; t < QT; ++t) {
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int qrow = q0 + t * QBLK + (lane >> 4) * 4 + r;
        if (qrow < S) {
          const float denom = l_run[t][r] > 0.f ? l_run[t][r] : 1.f;
          const int d = nb * 16 + (lane & 15);
          out[(((long)b * S + qrow) * H + h) * D + d] =
              f2bf(o_acc[t][nb][r] / denom);
        }
      }
    }
  }
}

// ------------------------------------------------------------ decode attn
// q [B, H, D], k/v cache [B, Hkv, Smax, D], seq_lens [B] -> out [B, H, D].
#define DEC_CHUNK 256   // keys per online-softmax chunk == threads per block
#define DEC_MAXG 8      // max query heads per kv head handled by one block

// GQA-aware: one block per (batch, kv-head) streams the KV cache ONCE and
// serves all G = H/Hkv query heads of the group — 1/G the HBM traffic of a
// block-per-query-head layout.  Template on G so per-thread accumulator
// arrays stay in registers (guide §5.4 rule 20).
// Split-S ("flash-decoding") contract: grid (Hkv, B, SPLITS); each split
// takes a contiguous 1/SPLITS of the VALID range [0, seq_lens[b]) (not of
// Smax: splitting the allocation left the low splits with full spans and
// the tail split nearly idle), streams it once for all G heads and writes
// UNNORMALIZED partials to the workspace
//   ws_o  [B, Hkv, SPLITS, G, D]   o = sum exp(s - m) v
//   ws_ml [B, Hkv, SPLITS, G, 2]   running max m, sum l (m = -inf: empty)
// which decode_attn_combine_kernel reduces.  SPLITS is chosen to fill the
// 256 CUs (Hkv*B alone is 0.5 blocks/CU at common shapes).  At SPLITS == 1
// (the 64-slot continuous-serving shape: B*Hkv already fills the chip) the
// block normalizes and writes `out` itself — no combine launch, no fp32
// workspace round-trip.
// DT: compile-time head dim.  Every inner loop gets a compile-time trip
// count so the compiler unrolls and BATCHES the global loads — the dynamic
// version compiled to ONE load + s_waitcnt(0) per iteration (zero
// memory-level parallelism; measured 87 us where streaming SoL is ~17 us).
// Phase A loads K rows COOPERATIVELY — a 16-lane group reads one 256 B row
// per iteration (1 KB coalesced per wave-instruction), each lane dots its
// 8-dim slice against its loop-invariant register copy of q (8 dims x G
// heads), group16 shuffles reduce the partials.  Phase B: a thread owns 8
// dims of every 16th key row (16 B V loads); its partial O accumulates
// across ALL chunks, rescaled by alpha like the softmax state, and is
// LDS-reduced once at the end.  ~10 KB LDS, ~170 VGPRs: 3 blocks/CU.
// Measured dead ends, kept out: staging K through a 64 KB XOR-swizzled LDS
// tile (2 blocks/CU, PMC wave-state split 48% parked on waits/barriers,
// 8-13% slower across shapes); a cross-chunk register-pipelined K prefetch
// (-20%: the in-order vmcnt counter makes later V waits drain it, and the
// doubled VGPRs halved occupancy).
template <int G, int DT>
__launch_bounds__(DEC_CHUNK, 1)
__global__ void decode_attn_coop_kernel(
    const bf16* __restrict__ q, const bf16* __restrict__ kc,
    const bf16* __restrict__ vc,
    float* __restrict__ ws_o, float* __restrict__ ws_ml,
    bf16* __restrict__ out,
    const int* __restrict__ seq_lens,
    int H, int Hkv, int Smax, int D_, float scale, int splits) {
  constexpr int D = DT;
  constexpr int ROWB = D / 8;              // lanes that cover one K row
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* p_sh = reinterpret_cast<float*>(smem);            // [G][DEC_CHUNK]
  float* q_sh = p_sh + G * DEC_CHUNK;                      // [G][D]
  float* red = q_sh + G * D;                               // [32] scratch
  float* o_sh = red + 32;                                  // [G][D]

  const int hkv = blockIdx.x;
  const int b = blockIdx.y;
  const int split = blockIdx.z;
  const int slen = seq_lens[b];
  const int span = (slen + splits - 1) / splits;
  const int s_begin = split * span;
  const int s_end = min(slen, s_begin + span);
  const bf16* kb = kc + ((long)b * Hkv + hkv) * Smax * (long)D;
  const bf16* vb = vc + ((long)b * Hkv + hkv) * Smax * (long)D;

  for (int i = threadIdx.x; i < G * D; i += blockDim.x) {
    const int g = i / D, d = i % D;
    q_sh[i] = bf2f(q[((long)b * H + hkv * G + g) * D + d]);
    o_sh[i] = 0.f;
  }
  __syncthreads();

  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x / WAVE;
  const int li = lane & 15;                // lane-in-group: dim slice owner
  const int g4 = lane >> 4;                // group in wave: key owner
  // loop-invariant per-lane q slice (lanes beyond ROWB duplicate a slice
  // and are masked out of the reduction)
  float q_reg[G][8];
#pragma unroll
  for (int g = 0; g < G; ++g)
#pragma unroll
    for (int e = 0; e < 8; ++e)
      q_reg[g][e] = q_sh[g * D + (li % ROWB) * 8 + e];

  float m_run[G], l_run[G], alpha[G];
#pragma unroll
  for (int g = 0; g < G; ++g) { m_run[g] = -INFINITY; l_run[g] = 0.f; }

  const int dgroup = threadIdx.x & 15;
  const int jslot = threadIdx.x >> 4;
  const bool dg_ok = dgroup < ROWB;
  float o_part[G][8];
#pragma unroll
  for (int g = 0; g < G; ++g)
#pragma unroll
    for (int e = 0; e < 8; ++e) o_part[g][e] = 0.f;

  for (int s0 = s_begin; s0 < s_end; s0 += DEC_CHUNK) {
    const int chunk = min(DEC_CHUNK, s_end - s0);
    // ---- phase A: cooperative dot.  Wave w owns keys [w*64, w*64+64);
    // iteration u: group g4 covers key w*64 + u*4 + g4; lane li reads its
    // 16 B dim slice.  Loads clamp to the valid span (no exec-mask
    // predication: it forces conservative vmcnt(0) waits); out-of-range
    // keys are masked in the softmax via row >= chunk.
    constexpr int AIT = 64 / 4;            // iterations per wave
    constexpr int ABATCH = 8;              // K rows in flight
#pragma unroll
    for (int u0 = 0; u0 < AIT; u0 += ABATCH) {
      bf16x8 kr[ABATCH];
#pragma unroll
      for (int u = 0; u < ABATCH; ++u) {
        const long key = min((long)(s0 + wid * 64 + (u0 + u) * 4 + g4),
                             (long)(s_end - 1));
        kr[u] = nt_load8(reinterpret_cast<const short*>(kb + key * D) +
                         (li % ROWB) * 8);
      }
#pragma unroll
      for (int u = 0; u < ABATCH; ++u) {
        float part[G];
#pragma unroll
        for (int g = 0; g < G; ++g) {
          float acc = 0.f;
#pragma unroll
          for (int e = 0; e < 8; ++e)
            acc += bits2f(kr[u][e]) * q_reg[g][e];
          part[g] = (li < ROWB) ? acc : 0.f;
        }
#pragma unroll
        for (int g = 0; g < G; ++g) part[g] = group16_sum(part[g]);
        if (li == 0) {
          const int key_local = wid * 64 + (u0 + u) * 4 + g4;
#pragma unroll
          for (int g = 0; g < G; ++g)
            p_sh[g * DEC_CHUNK + key_local] = part[g] * scale;
        }
      }
    }
    __syncthreads();                       // scores visible to owners

    // ---- V prefetch, first half (second half issues mid-PV)
    constexpr int JT = DEC_CHUNK / 16;
    constexpr int JH = JT / 2;
    bf16x8 v8[JH];
    auto load_v = [&](int half) {
#pragma unroll
      for (int u = 0; u < JH; ++u) {
        const long j = min((long)(s0 + jslot + (half * JH + u) * 16),
                           (long)(s_end - 1));
        v8[u] = nt_load8(reinterpret_cast<const short*>(vb + j * D) +
                         dgroup * 8);
      }
    };
    if (dg_ok) load_v(0);

    // ---- softmax (thread-per-key; raw score from p_sh, p written back
    // in place — each thread touches only its own slot before the
    // publishing barrier)
    {
      const int row = threadIdx.x;
      float sc[G];
#pragma unroll
      for (int g = 0; g < G; ++g)
        sc[g] = (row < chunk) ? p_sh[g * DEC_CHUNK + row] : -INFINITY;
      float mx[G];
#pragma unroll
      for (int g = 0; g < G; ++g) mx[g] = sc[g];
      block_reduce_vec<G, true>(mx, red);
      float sums[G];
#pragma unroll
      for (int g = 0; g < G; ++g) {
        const float m_new = fmaxf(m_run[g], mx[g]);
        float a = (m_run[g] == -INFINITY) ? 0.f : __expf(m_run[g] - m_new);
        if (m_new == -INFINITY) a = 1.f;
        alpha[g] = a;
        const float p = (sc[g] != -INFINITY) ? __expf(sc[g] - m_new) : 0.f;
        p_sh[g * DEC_CHUNK + row] = p;
        sums[g] = p;
        m_run[g] = m_new;
      }
      block_reduce_vec<G, false>(sums, red);  // barrier also publishes p_sh
#pragma unroll
      for (int g = 0; g < G; ++g)
        l_run[g] = l_run[g] * alpha[g] + sums[g];
    }

    // ---- PV consume in two halves
#pragma unroll
    for (int g = 0; g < G; ++g)
#pragma unroll
      for (int e = 0; e < 8; ++e) o_part[g][e] *= alpha[g];
    if (dg_ok) {
#pragma unroll
      for (int half = 0; half < 2; ++half) {
        if (half) load_v(1);
#pragma unroll
        for (int u = 0; u < JH; ++u) {
          const int j = jslot + (half * JH + u) * 16;
          if (j >= chunk) continue;        // p is 0 there anyway
          float vf[8];
#pragma unroll
          for (int e = 0; e < 8; ++e) vf[e] = bits2f(v8[u][e]);
#pragma unroll
          for (int g = 0; g < G; ++g) {
            const float p = p_sh[g * DEC_CHUNK + j];
#pragma unroll
            for (int e = 0; e < 8; ++e) o_part[g][e] += p * vf[e];
          }
        }
      }
    }
    __syncthreads();
  }

  if (dg_ok) {
#pragma unroll
    for (int g = 0; g < G; ++g)
#pragma unroll
      for (int e = 0; e < 8; ++e)
        atomicAdd(&o_sh[g * D + dgroup * 8 + e], o_part[g][e]);
  }
  __syncthreads();

  if (splits == 1) {
    for (int i = threadIdx.x; i < G * D; i += blockDim.x) {
      const int g = i / D, d = i % D;
      const float den = l_run[g] > 0.f ? l_run[g] : 1.f;
      out[((long)b * H + hkv * G + g) * D + d] = f2bf(o_sh[i] / den);
    }
    return;
  }
  const long base = (((long)b * Hkv + hkv) * splits + split) * G;
  for (int i = threadIdx.x; i < G * D; i += blockDim.x) {
    const int g = i / D, d = i % D;
    ws_o[(base + g) * D + d] = o_sh[i];
  }
  if (threadIdx.x == 0) {
#pragma unroll
    for (int g = 0; g < G; ++g) {
      ws_ml[(base + g) * 2 + 0] = m_run[g];
      ws_ml[(base + g) * 2 + 1] = l_run[g];
    }
  }
}

// combine: one block per (b, h); threads over D
__global__ void decode_attn_combine_kernel(
    const float* __restrict__ ws_o, const float* __restrict__ ws_ml,
    bf16* __restrict__ out, int H, int G, int D, int splits) {
  const int h = blockIdx.x;
  const int b = blockIdx.y;
  const int hkv = h / G;
  const int g = h % G;
  const long base0 = (((long)b * (H / G) + hkv) * splits) * G + g;
  // global max over splits
  float M = -INFINITY;
  for (int s = 0; s < splits; ++s)
    M = fmaxf(M, ws_ml[(base0 + (long)s * G) * 2 + 0]);
  float den = 0.f;
  for (int s = 0; s < splits; ++s) {
    const float m = ws_ml[(base0 + (long)s * G) * 2 + 0];
    const float l = ws_ml[(base0 + (long)s * G) * 2 + 1];
    if (m != -INFINITY) den += l * __expf(m - M);
  }
  if (den <= 0.f) den = 1.f;
  for (int d = threadIdx.x; d < D; d += blockDim.x) {
    float num = 0.f;
    for (int s = 0; s < splits; ++s) {
      const float m = ws_ml[(base0 + (long)s * G) * 2 + 0];
      if (m != -INFINITY)
        num += ws_o[(base0 + (long)s * G) * D + d] * __expf(m - M);
    }
    out[((long)b * H + h) * D + d] = f2bf(num / den);
  }
}

// One launcher for both prefill entry points: CACHE_SRC picks the K/V
// layout, plain prefill passes Smax = q_off = 0.
template <bool CACHE_SRC>
static hipError_t launch_flash_attn(const void* q, const void* k,
                                    const void* v, void* out,
                                    const int* kv_lens, int B, int S, int H,
                                    int Hkv, int D, float scale, int causal,
                                    int Smax, int q_off, hipStream_t stream) {
  size_t lds = (size_t)KVBLK * D * 2 * 2   // K (swizzled) + V (tr image)
               + FA_WAVES * FA_QT * QBLK * P_STRIDE;
  const int wave_rows = FA_QT * QBLK;
  dim3 grid((S + FA_WAVES * wave_rows - 1) / (FA_WAVES * wave_rows), H, B);
#define FA_CASE(DV)                                                          \
  case DV:                                                                   \
    hipLaunchKernelGGL((flash_attn_kernel<DV, CACHE_SRC>), grid,             \
                       dim3(FA_WAVES * WAVE), lds,                           \
                       stream, (const bf16*)q, (const bf16*)k,               \
                       (const bf16*)v, (bf16*)out, kv_lens, B, S, H, Hkv, D, \
                       scale, causal, Smax, q_off);                          \
    break;
  switch (D) {
    FA_CASE(32) FA_CASE(64) FA_CASE(96) FA_CASE(128)
    default:
      return hipErrorInvalidValue;
  }
#undef FA_CASE
  HIP_CHECK_LAUNCH();
  return hipSuccess;
}

extern "C" {

hipError_t sentio_flash_attn(const void* q, const void* k, const void* v,
                             void* out, const int* kv_lens, int B, int S,
                             int H, int Hkv, int D, float scale, int causal,
                             hipStream_t stream) {
  return launch_flash_attn<false>(q, k, v, out, kv_lens, B, S, H, Hkv, D,
                                  scale, causal, 0, 0, stream);
}

hipError_t sentio_flash_attn_cache(const void* q, const void* kc,
                                   const void* vc, void* out,
                                   const int* kv_lens, int B, int S, int H,
                                   int Hkv, int Smax, int D, float scale,
                                   int q_off, hipStream_t stream) {
  return launch_flash_attn<true>(q, kc, vc, out, kv_lens, B, S, H, Hkv, D,
                                 scale, 1, Smax, q_off, stream);
}

hipError_t sentio_decode_attn(const void* q, const void* kc, const void* vc,
                              void* out, const int* seq_lens,
                              float* ws_o, float* ws_ml, int splits,
                              int B, int H, int Hkv, int Smax, int D,
                              float scale, hipStream_t stream) {
  const int G = H / Hkv;
  if (H % Hkv || G > DEC_MAXG || (D != 64 && D != 128))
    return hipErrorInvalidValue;
  // p_sh [G][DEC_CHUNK] | q_sh [G][D] | red [32] | o_sh [G][D]
  const size_t lds = (size_t)(G * DEC_CHUNK + 2 * G * D + 32) * sizeof(float);
  dim3 grid(Hkv, B, splits);
#define DEC_CASE(GV, DV)                                                      \
  case GV * 1000 + DV:                                                        \
    hipLaunchKernelGGL((decode_attn_coop_kernel<GV, DV>), grid,               \
                       dim3(DEC_CHUNK), lds, stream, (const bf16*)q,          \
                       (const bf16*)kc, (const bf16*)vc, ws_o, ws_ml,         \
                       (bf16*)out, seq_lens, H, Hkv, Smax, D, scale, splits); \
    break;
#define DEC_ALL_G(DV)                                                 \
  DEC_CASE(1, DV) DEC_CASE(2, DV) DEC_CASE(3, DV) DEC_CASE(4, DV)     \
  DEC_CASE(5, DV) DEC_CASE(6, DV) DEC_CASE(7, DV) DEC_CASE(8, DV)
  switch (G * 1000 + D) {
    DEC_ALL_G(64) DEC_ALL_G(128)
    default:   // G < 1
      return hipErrorInvalidValue;
  }
#undef DEC_ALL_G
#undef DEC_CASE
  HIP_CHECK_LAUNCH();
  if (splits > 1) {   // splits==1 normalized + wrote out in the decode kernel
    hipLaunchKernelGGL(decode_attn_combine_kernel, dim3(H, B), dim3(128), 0,
                       stream, ws_o, ws_ml, (bf16*)out, H, G, D, splits);
    HIP_CHECK_LAUNCH();
  }
  return hipSuccess;
}

}  // extern "C"

