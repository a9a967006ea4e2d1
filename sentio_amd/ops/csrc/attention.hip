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
//    wave-private online softmax (no LDS or barrier in the key loop); a
//    combine kernel reduces the splits when there is more than one.  The
//    fused variant also applies RoPE and appends the new token's k/v row.
//  * decode_attn_fp8 / kv_store_fp8 — the opt-in FP8 (e4m3fn) KV cache: the
//    fused decode kernel over uint8 caches with static per-kv-head scales,
//    and the quantising splice of bf16 prefill K/V into such a cache.
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
#define DEC_MAXG 8      // max query heads per kv head handled by one block

// GQA-aware: one block per (batch, kv-head, split) streams its key span of
// the KV cache ONCE and serves all G = H/Hkv query heads of the group — 1/G
// the HBM traffic of a block-per-query-head layout.  Template on G, D and
// the block width NW (waves) so every per-thread array stays in registers
// and every inner loop has a compile-time trip count (a dynamic one
// compiled to ONE load + s_waitcnt(0) per iteration: 87 us where streaming
// SoL is ~17 us).
//
// Wave-private online softmax — no LDS and no barrier in the key loop.
// In a wave, lane li = lane & 15 owns dims [li*8, li*8+8) and the 16-lane
// group g4 = lane >> 4 owns one key per load instruction: four consecutive
// cache rows per wave-instruction, 1 KB coalesced at D=128.  A lane loads
// 16 B of K and 16 B of V of the SAME key, dots its K slice against its
// register copy of q (pre-multiplied by scale*log2 e), a DPP butterfly
// leaves the score in all 16 lanes of the group, and the group keeps its
// OWN running max m[G], sum l[G] and its dim slice of O, o[G][8], updated
// from its own keys only.  The max update and the rescale run once per
// batch of KB keys per group; the batch's 2*KB loads issue back to back
// before the first use, K first, so the waits are counted and V is still
// in flight while the scores are formed.  Waves take batches of the block's
// span interleaved (wave w: batches w, w+NW, ...), so a ragged span keeps
// every wave busy to its end.  Loads clamp to the span (no exec-mask
// predication: it forces conservative vmcnt(0) waits); clamped keys are
// masked to -inf.  Once per block the four groups of a wave fold through
// __shfl_xor 16/32 and the waves through NW*(G*D + 2G) floats of LDS with
// a single barrier; every fold treats m = -inf (a group, wave or split
// that owned no key) as weight 0, and l = 0 writes zeros.
//
// Split-S ("flash-decoding") contract: grid (Hkv, B, SPLITS); each split
// takes a contiguous 1/SPLITS of the VALID range (not of Smax: splitting
// the allocation left the low splits with full spans and the tail split
// nearly idle) and writes UNNORMALIZED partials to the workspace
//   ws_o  [B, Hkv, SPLITS, G, D]   o = sum exp(s - m) v
//   ws_ml [B, Hkv, SPLITS, G, 2]   running max m, sum l (m = -inf: empty)
// which decode_attn_combine_kernel reduces.  At SPLITS == 1 the block
// normalizes and writes `out` itself — no combine launch, no fp32
// workspace round-trip; the wave-private state makes a wider block free, so
// the launcher (bindings.hip) takes 8 waves instead of 2 splits once
// B*Hkv fills the chip.
//
// FUSED: the q source is the raw QKV projection [B, (H+2*Hkv)*D] and
// seq_lens[b] is the position `pos` of the new token.  Every lane rotates
// its own q slice (RoPE at pos; its 8 dims are 4 whole pairs) and rounds
// it to bf16 exactly as decode_qkv_prep_kernel does, so no q tensor
// exists.  Keys [0, pos) stream from the cache; the block of the LAST
// split rotates and rounds the new k, stores the new k/v rows at row pos
// and seeds wave 0 / group 0's softmax state with that key from
// registers.  No block reads row pos in this launch, rows < pos are never
// written.  The rotation is written with explicit fma/mul in the order the
// prep kernel compiles to, so the stored K row is bit-equal to its.
//
// Measured (profiles/README.md "Wave-private decode attention"): isolated,
// llama3-8b heads, B=32 slen=1600 (210 MB of K+V): 37.4 us = 5.6 TB/s,
// against 82.0 us for the block-shared kernel before it; B=16: 26 us
// against 56; B=32 slen=512: 15 us against 41.  In the bench's decode graph
// the attention chain (prep + attention + combine) went from 68.7 to
// 24.6 us per layer at batch 32 and from 54.7 to 23.4 us at batch 16.
// <4,128>: 237 VGPRs (188 fused), no scratch, 2 waves/SIMD at NW 4 and 8 —
// what one 8-wave block per CU provides anyway; NW=16 would cap a wave at
// 128 VGPRs and is not instantiated.  KB shrinks with G so that every
// instantiation stays free of scratch.
//
// Measured dead ends, kept out: block-shared softmax state (scores through
// an LDS p_sh, two block reductions per 256-key chunk: ~6 barriers per
// chunk, PMC 48% of wave time parked on waits/barriers); staging K through
// a 64 KB XOR-swizzled LDS tile (2 blocks/CU, 8-13% slower across shapes);
// a cross-chunk K-only register prefetch (-20%: with V loads between, the
// in-order vmcnt counter made later V waits drain it, and the doubled
// VGPRs halved occupancy).
template <int CTRL>
__device__ __forceinline__ float dpp_mov(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(
      0, __float_as_int(v), CTRL, 0xf, 0xf, true));
}
// sum within 16-lane rows on the VALU (DPP), result in every lane: xor 1 and
// xor 2 as quad permutes, then half-row and row mirrors (quads, then
// halves, already hold equal values, so a mirror acts as xor 4 / xor 8).
// __shfl_xor would go through the LDS crossbar (ds_bpermute).
__device__ __forceinline__ float group16_sum_dpp(float v) {
  v += dpp_mov<0xB1>(v);    // quad_perm [1,0,3,2]
  v += dpp_mov<0x4E>(v);    // quad_perm [2,3,0,1]
  v += dpp_mov<0x141>(v);   // row_half_mirror
  v += dpp_mov<0x140>(v);   // row_mirror
  return v;
}
__device__ __forceinline__ float fast_exp2(float x) {
  return __builtin_amdgcn_exp2f(x);       // v_exp_f32; exp2(-inf) = 0
}
// RoPE on one lane's 8-dim slice (4 pairs), rounded to bf16 bits.  Same
// operation order as decode_qkv_prep_kernel's compiled form:
//   y0 = fma(x0, c, -(x1*sn)),  y1 = fma(x1, c, x0*sn).
__device__ __forceinline__ bf16x8 rope_slice(bf16x8 x, const float4 c,
                                             const float4 sn) {
  const float cc[4] = {c.x, c.y, c.z, c.w};
  const float ss[4] = {sn.x, sn.y, sn.z, sn.w};
  bf16x8 y;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float x0 = bits2f(x[2 * j]), x1 = bits2f(x[2 * j + 1]);
    const float y0 = __builtin_fmaf(x0, cc[j], -(x1 * ss[j]));
    const float y1 = __builtin_fmaf(x1, cc[j], x0 * ss[j]);
    const bf16 r0 = f2bf(y0), r1 = f2bf(y1);
    y[2 * j] = (short)__builtin_bit_cast(unsigned short, r0);
    y[2 * j + 1] = (short)__builtin_bit_cast(unsigned short, r1);
  }
  return y;
}

// keys per group per batch: 2*KB 16-byte loads in flight per lane
// (sized so q, o, the scores and the batch fit 256 VGPRs without scratch)
template <int G> struct DecBatch {
  static constexpr int value = G <= 4 ? 8 : G <= 6 ? 4 : 2;
};

template <int G, int DT, int NW, bool FUSED>
__launch_bounds__(NW * WAVE)
__global__ void decode_attn_kernel(
    const bf16* __restrict__ qsrc, bf16* kc, bf16* vc,
    float* __restrict__ ws_o, float* __restrict__ ws_ml,
    bf16* __restrict__ out,
    const float* __restrict__ cosT, const float* __restrict__ sinT,
    const int* __restrict__ seq_lens,
    int H, int Hkv, int Smax, float scale, int splits) {
  constexpr int D = DT;
  constexpr int ROWB = D / 8;              // lanes that cover one K row
  constexpr int KB = DecBatch<G>::value;
  constexpr float LOG2E = 1.4426950408889634f;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* sm_o = reinterpret_cast<float*>(smem);            // [NW][G][D]
  float* sm_ml = sm_o + NW * G * D;                        // [NW][G][2]

  const int hkv = blockIdx.x;
  const int b = blockIdx.y;
  const int split = blockIdx.z;
  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE);
  const int li = lane & 15;                // lane-in-group: dim slice owner
  const int g4 = lane >> 4;                // group in wave: key owner
  // lanes beyond ROWB (D=64) duplicate a slice and are masked out of the dot
  const int ls = li % ROWB;
  const int len_raw = seq_lens[b];
  const int slen = max(0, min(len_raw, Smax));   // cache rows to stream
  const int span = (slen + splits - 1) / splits;
  const int s_begin = split * span;
  const int s_end = min(slen, s_begin + span);
  const long cache_off = ((long)b * Hkv + hkv) * Smax * (long)D;
  const short* kb = reinterpret_cast<const short*>(kc + cache_off) + ls * 8;
  const short* vb = reinterpret_cast<const short*>(vc + cache_off) + ls * 8;

  // ---- q slice: loop-invariant registers, pre-scaled for exp2
  const int HT = FUSED ? H + 2 * Hkv : H;  // heads per row of qsrc
  const int pos = max(0, min(len_raw, Smax - 1));
  float4 rc, rs;
  if (FUSED) {
    const long toff = (long)pos * (D / 2) + ls * 4;
    rc = *reinterpret_cast<const float4*>(cosT + toff);
    rs = *reinterpret_cast<const float4*>(sinT + toff);
  }
  const float qs = scale * LOG2E;
  float q_reg[G][8];
#pragma unroll
  for (int g = 0; g < G; ++g) {
    bf16x8 qv = *reinterpret_cast<const bf16x8*>(
        qsrc + ((long)b * HT + hkv * G + g) * D + ls * 8);
    if (FUSED) qv = rope_slice(qv, rc, rs);
#pragma unroll
    for (int e = 0; e < 8; ++e) q_reg[g][e] = bits2f(qv[e]) * qs;
  }

  float m_run[G], l_run[G], o[G][8];
#pragma unroll
  for (int g = 0; g < G; ++g) {
    m_run[g] = -INFINITY;
    l_run[g] = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) o[g][e] = 0.f;
  }

  // ---- FUSED: the new token, owned by the last split's block
  if (FUSED && split == splits - 1) {
    const bf16* krow = qsrc + ((long)b * HT + H + hkv) * D + ls * 8;
    bf16x8 kn = rope_slice(*reinterpret_cast<const bf16x8*>(krow), rc, rs);
    const bf16x8 vn = *reinterpret_cast<const bf16x8*>(krow + (long)Hkv * D);
    const bool take = wid == 0 && g4 == 0;
    if (take && li < ROWB && len_raw >= 0 && len_raw < Smax) {
      const long row = cache_off + (long)len_raw * D + li * 8;
      *reinterpret_cast<bf16x8*>(kc + row) = kn;
      *reinterpret_cast<bf16x8*>(vc + row) = vn;
    }
    float sn[G];
#pragma unroll
    for (int g = 0; g < G; ++g) {
      float acc = 0.f;
#pragma unroll
      for (int e = 0; e < 8; ++e) acc += bits2f(kn[e]) * q_reg[g][e];
      if (ROWB < 16) acc = (li < ROWB) ? acc : 0.f;
      sn[g] = group16_sum_dpp(acc);
    }
    if (take) {                            // p = exp2(s - s) = 1
#pragma unroll
      for (int g = 0; g < G; ++g) {
        m_run[g] = sn[g];
        l_run[g] = 1.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) o[g][e] = bits2f(vn[e]);
      }
    }
  }

  // ---- key loop: wave-private, no LDS, no barrier
  const int nbatch = (s_end - s_begin + 4 * KB - 1) / (4 * KB);
  for (int t = wid; t < nbatch; t += NW) {
    const int k0 = s_begin + t * (4 * KB) + g4;
    bf16x8 kr[KB], vr[KB];
#pragma unroll
    for (int u = 0; u < KB; ++u)
      kr[u] = nt_load8(kb + (long)min(k0 + u * 4, s_end - 1) * D);
#pragma unroll
    for (int u = 0; u < KB; ++u)
      vr[u] = nt_load8(vb + (long)min(k0 + u * 4, s_end - 1) * D);
    // keep all 2*KB loads ahead of the first use: left alone, the scheduler
    // sinks each V load next to its consumer behind a vmcnt(0)
    __builtin_amdgcn_sched_barrier(0);

    float s[KB][G];
#pragma unroll
    for (int u = 0; u < KB; ++u) {
#pragma unroll
      for (int g = 0; g < G; ++g) {
        float acc = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) acc += bits2f(kr[u][e]) * q_reg[g][e];
        if (ROWB < 16) acc = (li < ROWB) ? acc : 0.f;
        acc = group16_sum_dpp(acc);
        s[u][g] = (k0 + u * 4 < s_end) ? acc : -INFINITY;
      }
    }
#pragma unroll
    for (int g = 0; g < G; ++g) {
      float mx = s[0][g];
#pragma unroll
      for (int u = 1; u < KB; ++u) mx = fmaxf(mx, s[u][g]);
      const float m_new = fmaxf(m_run[g], mx);
      const float m_safe = (m_new == -INFINITY) ? 0.f : m_new;
      const float alpha = fast_exp2(m_run[g] - m_safe);
      m_run[g] = m_new;
      float l = l_run[g] * alpha;
#pragma unroll
      for (int e = 0; e < 8; ++e) o[g][e] *= alpha;
#pragma unroll
      for (int u = 0; u < KB; ++u) {
        const float p = fast_exp2(s[u][g] - m_safe);
        s[u][g] = p;
        l += p;
      }
      l_run[g] = l;
    }
#pragma unroll
    for (int u = 0; u < KB; ++u) {
      float vf[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) vf[e] = bits2f(vr[u][e]);
#pragma unroll
      for (int g = 0; g < G; ++g)
#pragma unroll
        for (int e = 0; e < 8; ++e) o[g][e] += s[u][g] * vf[e];
    }
  }

  // ---- fold the wave's four groups (same dim slice, different keys)
#pragma unroll
  for (int off = 16; off <= 32; off <<= 1) {
#pragma unroll
    for (int g = 0; g < G; ++g) {
      const float mo = __shfl_xor(m_run[g], off, WAVE);
      const float lo = __shfl_xor(l_run[g], off, WAVE);
      const float mm = fmaxf(m_run[g], mo);
      const float ms = (mm == -INFINITY) ? 0.f : mm;
      const float a = fast_exp2(m_run[g] - ms);
      const float ao = fast_exp2(mo - ms);
      l_run[g] = l_run[g] * a + lo * ao;
#pragma unroll
      for (int e = 0; e < 8; ++e)
        o[g][e] = o[g][e] * a + __shfl_xor(o[g][e], off, WAVE) * ao;
      m_run[g] = mm;
    }
  }

  // ---- fold the waves through LDS, one barrier
  if (g4 == 0 && li < ROWB) {
#pragma unroll
    for (int g = 0; g < G; ++g) {
      float4* dst =
          reinterpret_cast<float4*>(sm_o + (wid * G + g) * D + li * 8);
      dst[0] = make_float4(o[g][0], o[g][1], o[g][2], o[g][3]);
      dst[1] = make_float4(o[g][4], o[g][5], o[g][6], o[g][7]);
    }
  }
  if (lane == 0) {
#pragma unroll
    for (int g = 0; g < G; ++g) {
      sm_ml[(wid * G + g) * 2 + 0] = m_run[g];
      sm_ml[(wid * G + g) * 2 + 1] = l_run[g];
    }
  }
  __syncthreads();

  const long base = (((long)b * Hkv + hkv) * splits + split) * G;
  for (int i = threadIdx.x; i < G * D; i += NW * WAVE) {
    const int g = i / D, d = i % D;
    float M = -INFINITY;
#pragma unroll
    for (int w = 0; w < NW; ++w) M = fmaxf(M, sm_ml[(w * G + g) * 2]);
    const float ms = (M == -INFINITY) ? 0.f : M;
    float num = 0.f, den = 0.f;
#pragma unroll
    for (int w = 0; w < NW; ++w) {
      const float a = fast_exp2(sm_ml[(w * G + g) * 2] - ms);
      den += sm_ml[(w * G + g) * 2 + 1] * a;
      num += sm_o[(w * G + g) * D + d] * a;
    }
    if (splits == 1) {
      out[((long)b * H + hkv * G + g) * D + d] =
          f2bf(den > 0.f ? num / den : 0.f);
    } else {
      ws_o[(base + g) * D + d] = num;
      if (d == 0) {                        // m back in natural-log units
        ws_ml[(base + g) * 2 + 0] = M * (1.f / LOG2E);
        ws_ml[(base + g) * 2 + 1] = den;
      }
    }
  }
}

// ------------------------------------------------------------ FP8 KV cache
// Opt-in e4m3fn (OCP, = torch.float8_e4m3fn) cache: uint8 [B, Hkv, Smax, D]
// with static fp32 scales per kv head.  Quantisation is
//   byte = RNE_e4m3fn(clamp(fp32(x) * inv, -448, +448))
// with the clamp done in fp32 ahead of v_cvt_pk_fp8_f32 (no reliance on a
// saturation mode bit), so a finite input never yields 0x7F / 0xFF.  The
// kernels only multiply: inv = 1/scale is computed once on the host side.
typedef unsigned u32x2_t __attribute__((ext_vector_type(2)));
typedef unsigned u32x4_t __attribute__((ext_vector_type(4)));
typedef float f32x2_t __attribute__((ext_vector_type(2)));
#define FP8_E4M3_MAX 448.f

__device__ __forceinline__ float fp8_clamp(float x) {
  return __builtin_fminf(__builtin_fmaxf(x, -FP8_E4M3_MAX), FP8_E4M3_MAX);
}
// 8 bf16 (raw bits) * inv -> 8 e4m3fn bytes, element e in byte e
__device__ __forceinline__ u32x2_t fp8_quant8(bf16x8 x, float inv) {
  float f[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) f[e] = fp8_clamp(bits2f(x[e]) * inv);
  int lo = __builtin_amdgcn_cvt_pk_fp8_f32(f[0], f[1], 0, false);
  lo = __builtin_amdgcn_cvt_pk_fp8_f32(f[2], f[3], lo, true);
  int hi = __builtin_amdgcn_cvt_pk_fp8_f32(f[4], f[5], 0, false);
  hi = __builtin_amdgcn_cvt_pk_fp8_f32(f[6], f[7], hi, true);
  u32x2_t r;
  r.x = (unsigned)lo;
  r.y = (unsigned)hi;
  return r;
}
// 8 e4m3fn bytes -> 8 floats (unscaled): four v_cvt_pk_f32_fp8
__device__ __forceinline__ void fp8_unpack8(u32x2_t w, float (&f)[8]) {
  const f32x2_t a = __builtin_amdgcn_cvt_pk_f32_fp8((int)w.x, false);
  const f32x2_t b = __builtin_amdgcn_cvt_pk_f32_fp8((int)w.x, true);
  const f32x2_t c = __builtin_amdgcn_cvt_pk_f32_fp8((int)w.y, false);
  const f32x2_t d = __builtin_amdgcn_cvt_pk_f32_fp8((int)w.y, true);
  f[0] = a.x; f[1] = a.y; f[2] = b.x; f[3] = b.y;
  f[4] = c.x; f[5] = c.y; f[6] = d.x; f[7] = d.y;
}

// 8 or 16 e4m3fn bytes per lane and key: one 8 B / 16 B non-temporal load
template <int EPL> struct Fp8Row;
template <> struct Fp8Row<8> {
  u32x2_t w;
  __device__ __forceinline__ void load(const unsigned char* p) {
    w = __builtin_nontemporal_load(reinterpret_cast<const u32x2_t*>(p));
  }
  __device__ __forceinline__ void store(unsigned char* p) const {
    *reinterpret_cast<u32x2_t*>(p) = w;
  }
  __device__ __forceinline__ u32x2_t chunk(int) const { return w; }
  __device__ __forceinline__ void set(int, u32x2_t v) { w = v; }
};
template <> struct Fp8Row<16> {
  u32x4_t w;
  __device__ __forceinline__ void load(const unsigned char* p) {
    w = __builtin_nontemporal_load(reinterpret_cast<const u32x4_t*>(p));
  }
  __device__ __forceinline__ void store(unsigned char* p) const {
    *reinterpret_cast<u32x4_t*>(p) = w;
  }
  __device__ __forceinline__ u32x2_t chunk(int c) const {
    u32x2_t r;
    r.x = c ? w.z : w.x;
    r.y = c ? w.w : w.y;
    return r;
  }
  __device__ __forceinline__ void set(int c, u32x2_t v) {
    if (c) { w.z = v.x; w.w = v.y; } else { w.x = v.x; w.y = v.y; }
  }
};
template <int EPL>
__device__ __forceinline__ void fp8_unpack_row(const Fp8Row<EPL>& r,
                                               float (&f)[EPL]) {
#pragma unroll
  for (int c = 0; c < EPL / 8; ++c) {
    float t[8];
    fp8_unpack8(r.chunk(c), t);
#pragma unroll
    for (int e = 0; e < 8; ++e) f[c * 8 + e] = t[e];
  }
}
// sum over the LPK (16 or 8) lanes of a key, result in every lane
template <int LPK>
__device__ __forceinline__ float key_sum_dpp(float v) {
  v += dpp_mov<0xB1>(v);    // quad_perm [1,0,3,2]
  v += dpp_mov<0x4E>(v);    // quad_perm [2,3,0,1]
  v += dpp_mov<0x141>(v);   // row_half_mirror
  if (LPK == 16) v += dpp_mov<0x140>(v);   // row_mirror
  return v;
}

// Elements per lane of the FP8 kernel.  8: the (li, g4) mapping of the bf16
// kernel, 16 lanes and an 8 B load per key, 4 keys per wave instruction.
// 16 (D = 128, G <= 4): 8 lanes and a 16 B load per key, 8 keys per wave
// instruction, an 8-lane DPP sum — half the reduction work per key, but q
// and o take 32 registers per query head, which fits without scratch only
// up to G = 4.  Measured, llama3-8b heads (profiles/kv_fp8.md): 16 is 9-12%
// faster at 1600 keys and 8% slower at 512; both beat the bf16 kernel.
template <int G, int DT> struct Fp8Epl {
  static constexpr int value = (DT == 128 && G <= 4) ? 16 : 8;
};

// FP8 sibling of decode_attn_kernel<FUSED> (the bf16 instantiations are not
// touched): same grid, split, wave and seq_lens contract.  A key's row is
// covered by LPK lanes of EPL dims each; a lane loads EPL bytes of K and of
// V per key and unpacks them with v_cvt_pk_f32_fp8.  A batch is two halves
// of SUB keys per lane group (one at G = 8): all loads of both halves issue
// back to back, in the order they are consumed, then the softmax update
// runs per half, so the score registers stay those of the bf16 kernel (one
// update over the whole batch spilled to scratch at G >= 4).  At EPL = 8 a
// batch holds the bf16 kernel's load registers and bytes in flight.
//   * the new k row is rotated and rounded to bf16 exactly as the bf16
//     fused kernel stores it, then quantised; the bytes stored are
//     quantise(that row).  v likewise.
//   * the new token enters its own attention as the DEQUANTISED stored
//     value: this step sees the K/V every later step will read.
//   * k_scale folds into the pre-scaled q registers; v_scale multiplies the
//     reduced numerator, both at splits == 1 and in the ws_o partials, so
//     decode_attn_combine_kernel and the ws_ml contract are unchanged.
// scales are read at run time (in-place updates need no graph recapture).
template <int G, int DT, int NW, int EPL>
__launch_bounds__(NW * WAVE)
__global__ void decode_attn_fp8_kernel(
    const bf16* __restrict__ qsrc, unsigned char* kc, unsigned char* vc,
    float* __restrict__ ws_o, float* __restrict__ ws_ml,
    bf16* __restrict__ out,
    const float* __restrict__ cosT, const float* __restrict__ sinT,
    const int* __restrict__ seq_lens,
    const float* __restrict__ k_scale, const float* __restrict__ v_scale,
    const float* __restrict__ k_inv, const float* __restrict__ v_inv,
    int H, int Hkv, int Smax, float scale, int splits) {
  constexpr int D = DT;
  constexpr int ROWB = D / EPL;            // lanes that cover one K row
  constexpr int LPK = EPL == 16 ? 8 : 16;  // lanes per key (>= ROWB)
  constexpr int KPW = WAVE / LPK;          // keys per wave instruction
  constexpr int NC = EPL / 8;              // 8-element chunks per lane
  static_assert(ROWB <= LPK, "row wider than its lane group");
  // EPL = 16 halves the sub-batch: its q, o and load registers are twice as
  // wide.  G = 8 keeps one half: q and o alone hold 128 registers there.
  constexpr int SUB = EPL == 16 ? 2 : DecBatch<G>::value;
  constexpr int HALVES = G <= 7 ? 2 : 1;
  constexpr int KB = HALVES * SUB;         // keys per lane group per batch
  constexpr float LOG2E = 1.4426950408889634f;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* sm_o = reinterpret_cast<float*>(smem);            // [NW][G][D]
  float* sm_ml = sm_o + NW * G * D;                        // [NW][G][2]

  const int hkv = blockIdx.x;
  const int b = blockIdx.y;
  const int split = blockIdx.z;
  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE);
  const int li = lane & (LPK - 1);         // lane-in-group: dim slice owner
  const int gk = lane / LPK;               // group in wave: key owner
  const int ls = li % ROWB;                // D=64: upper lanes duplicate
  const int len_raw = seq_lens[b];
  const int slen = max(0, min(len_raw, Smax));   // cache rows to stream
  const int span = (slen + splits - 1) / splits;
  const int s_begin = split * span;
  const int s_end = min(slen, s_begin + span);
  const long cache_off = ((long)b * Hkv + hkv) * Smax * (long)D;
  // block-uniform bases + one 32-bit lane offset shared by the K and V
  // load of a key (a (b, kv-head) slab is far below 4 GB): scalar base +
  // 1-VGPR offset addressing instead of a 64-bit address pair per load
  const unsigned char* kb = kc + cache_off;
  const unsigned char* vb = vc + cache_off;
  const int lo = ls * EPL;

  // ---- q slice: RoPE, bf16 rounding, pre-scaled by scale*log2e*k_scale
  const int HT = H + 2 * Hkv;
  const int pos = max(0, min(len_raw, Smax - 1));
  const long toff = (long)pos * (D / 2) + ls * (EPL / 2);
  float4 rc[NC], rs[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    rc[c] = *reinterpret_cast<const float4*>(cosT + toff + c * 4);
    rs[c] = *reinterpret_cast<const float4*>(sinT + toff + c * 4);
  }
  const float qs = scale * LOG2E * k_scale[hkv];
  float q_reg[G][EPL];
#pragma unroll
  for (int g = 0; g < G; ++g) {
    const bf16* qp = qsrc + ((long)b * HT + hkv * G + g) * D + lo;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const bf16x8 qv = rope_slice(
          *reinterpret_cast<const bf16x8*>(qp + c * 8), rc[c], rs[c]);
#pragma unroll
      for (int e = 0; e < 8; ++e) q_reg[g][c * 8 + e] = bits2f(qv[e]) * qs;
    }
  }

  float m_run[G], l_run[G], o[G][EPL];
#pragma unroll
  for (int g = 0; g < G; ++g) {
    m_run[g] = -INFINITY;
    l_run[g] = 0.f;
#pragma unroll
    for (int e = 0; e < EPL; ++e) o[g][e] = 0.f;
  }

  // ---- the new token, owned by the last split's block
  if (split == splits - 1) {
    const bf16* krow = qsrc + ((long)b * HT + H + hkv) * D + lo;
    const float ki = k_inv[hkv], vi = v_inv[hkv];
    Fp8Row<EPL> kq, vq;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const bf16x8 kn = rope_slice(
          *reinterpret_cast<const bf16x8*>(krow + c * 8), rc[c], rs[c]);
      const bf16x8 vn =
          *reinterpret_cast<const bf16x8*>(krow + (long)Hkv * D + c * 8);
      kq.set(c, fp8_quant8(kn, ki));
      vq.set(c, fp8_quant8(vn, vi));
    }
    const bool take = wid == 0 && gk == 0;
    if (take && li < ROWB && len_raw >= 0 && len_raw < Smax) {
      const long row = cache_off + (long)len_raw * D + li * EPL;
      kq.store(kc + row);
      vq.store(vc + row);
    }
    float kf[EPL], vf[EPL];
    fp8_unpack_row<EPL>(kq, kf);
    fp8_unpack_row<EPL>(vq, vf);
    float sn[G];
#pragma unroll
    for (int g = 0; g < G; ++g) {
      float acc = 0.f;
#pragma unroll
      for (int e = 0; e < EPL; ++e) acc += kf[e] * q_reg[g][e];
      if (ROWB < LPK) acc = (li < ROWB) ? acc : 0.f;
      sn[g] = key_sum_dpp<LPK>(acc);
    }
    if (take) {                            // p = exp2(s - s) = 1
#pragma unroll
      for (int g = 0; g < G; ++g) {
        m_run[g] = sn[g];
        l_run[g] = 1.f;
#pragma unroll
        for (int e = 0; e < EPL; ++e) o[g][e] = vf[e];
      }
    }
  }

  // ---- key loop: wave-private, no LDS, no barrier
  const int nbatch = (s_end - s_begin + KPW * KB - 1) / (KPW * KB);
  for (int t = wid; t < nbatch; t += NW) {
    const int k0 = s_begin + t * (KPW * KB) + gk;
    // issue order = consume order (K h0, V h0, K h1, V h1): the in-order
    // vmcnt waits then never drain loads that are not needed yet
    Fp8Row<EPL> kr[HALVES][SUB], vr[HALVES][SUB];
#pragma unroll
    for (int h = 0; h < HALVES; ++h) {
#pragma unroll
      for (int u = 0; u < SUB; ++u)
        kr[h][u].load(kb + (unsigned)(
            min(k0 + (h * SUB + u) * KPW, s_end - 1) * D + lo));
#pragma unroll
      for (int u = 0; u < SUB; ++u)
        vr[h][u].load(vb + (unsigned)(
            min(k0 + (h * SUB + u) * KPW, s_end - 1) * D + lo));
    }
    // all 2*KB loads ahead of the first use (see decode_attn_kernel)
    __builtin_amdgcn_sched_barrier(0);

#pragma unroll
    for (int h = 0; h < HALVES; ++h) {
      float s[SUB][G];
#pragma unroll
      for (int u = 0; u < SUB; ++u) {
        float kf[EPL];
        fp8_unpack_row<EPL>(kr[h][u], kf);
#pragma unroll
        for (int g = 0; g < G; ++g) {
          float acc = 0.f;
#pragma unroll
          for (int e = 0; e < EPL; ++e) acc += kf[e] * q_reg[g][e];
          if (ROWB < LPK) acc = (li < ROWB) ? acc : 0.f;
          acc = key_sum_dpp<LPK>(acc);
          s[u][g] = (k0 + (h * SUB + u) * KPW < s_end) ? acc : -INFINITY;
        }
      }
#pragma unroll
      for (int g = 0; g < G; ++g) {
        float mx = s[0][g];
#pragma unroll
        for (int u = 1; u < SUB; ++u) mx = fmaxf(mx, s[u][g]);
        const float m_new = fmaxf(m_run[g], mx);
        const float m_safe = (m_new == -INFINITY) ? 0.f : m_new;
        const float alpha = fast_exp2(m_run[g] - m_safe);
        m_run[g] = m_new;
        float l = l_run[g] * alpha;
#pragma unroll
        for (int e = 0; e < EPL; ++e) o[g][e] *= alpha;
#pragma unroll
        for (int u = 0; u < SUB; ++u) {
          const float p = fast_exp2(s[u][g] - m_safe);
          s[u][g] = p;
          l += p;
        }
        l_run[g] = l;
      }
#pragma unroll
      for (int u = 0; u < SUB; ++u) {
        float vf[EPL];
        fp8_unpack_row<EPL>(vr[h][u], vf);
#pragma unroll
        for (int g = 0; g < G; ++g)
#pragma unroll
          for (int e = 0; e < EPL; ++e) o[g][e] += s[u][g] * vf[e];
      }
      // the halves stay apart: interleaved, their unpacked floats and
      // scores are live together and the kernel spills
      __builtin_amdgcn_sched_barrier(0);
    }
  }

  // ---- fold the wave's lane groups (same dim slice, different keys)
#pragma unroll
  for (int off = LPK; off <= 32; off <<= 1) {
#pragma unroll
    for (int g = 0; g < G; ++g) {
      const float mo = __shfl_xor(m_run[g], off, WAVE);
      const float lo_ = __shfl_xor(l_run[g], off, WAVE);
      const float mm = fmaxf(m_run[g], mo);
      const float ms = (mm == -INFINITY) ? 0.f : mm;
      const float a = fast_exp2(m_run[g] - ms);
      const float ao = fast_exp2(mo - ms);
      l_run[g] = l_run[g] * a + lo_ * ao;
#pragma unroll
      for (int e = 0; e < EPL; ++e)
        o[g][e] = o[g][e] * a + __shfl_xor(o[g][e], off, WAVE) * ao;
      m_run[g] = mm;
    }
  }

  // ---- fold the waves through LDS, one barrier
  if (gk == 0 && li < ROWB) {
#pragma unroll
    for (int g = 0; g < G; ++g) {
      float4* dst =
          reinterpret_cast<float4*>(sm_o + (wid * G + g) * D + li * EPL);
#pragma unroll
      for (int j = 0; j < EPL / 4; ++j)
        dst[j] = make_float4(o[g][4 * j], o[g][4 * j + 1], o[g][4 * j + 2],
                             o[g][4 * j + 3]);
    }
  }
  if (lane == 0) {
#pragma unroll
    for (int g = 0; g < G; ++g) {
      sm_ml[(wid * G + g) * 2 + 0] = m_run[g];
      sm_ml[(wid * G + g) * 2 + 1] = l_run[g];
    }
  }
  __syncthreads();

  const float vs = v_scale[hkv];
  const long base = (((long)b * Hkv + hkv) * splits + split) * G;
  for (int i = threadIdx.x; i < G * D; i += NW * WAVE) {
    const int g = i / D, d = i % D;
    float M = -INFINITY;
#pragma unroll
    for (int w = 0; w < NW; ++w) M = fmaxf(M, sm_ml[(w * G + g) * 2]);
    const float ms = (M == -INFINITY) ? 0.f : M;
    float num = 0.f, den = 0.f;
#pragma unroll
    for (int w = 0; w < NW; ++w) {
      const float a = fast_exp2(sm_ml[(w * G + g) * 2] - ms);
      den += sm_ml[(w * G + g) * 2 + 1] * a;
      num += sm_o[(w * G + g) * D + d] * a;
    }
    num *= vs;
    if (splits == 1) {
      out[((long)b * H + hkv * G + g) * D + d] =
          f2bf(den > 0.f ? num / den : 0.f);
    } else {
      ws_o[(base + g) * D + d] = num;
      if (d == 0) {                        // m back in natural-log units
        ws_ml[(base + g) * 2 + 0] = M * (1.f / LOG2E);
        ws_ml[(base + g) * 2 + 1] = den;
      }
    }
  }
}

// Quantising splice: the first S rows of each bf16 source row
// [n, Hkv, S_src, D] go to dst[rows[i], :, :S, :] of the uint8 caches
// [B, Hkv, Smax, D]; K and V in one launch.  One thread per 8 elements:
// a 16 B load and an 8 B store per tensor.  rows[i] outside [0, B) is
// skipped; nothing is written beyond S or Smax.
__global__ void kv_store_fp8_kernel(
    const bf16* __restrict__ src_k, const bf16* __restrict__ src_v,
    unsigned char* __restrict__ dst_k, unsigned char* __restrict__ dst_v,
    const int* __restrict__ rows, const float* __restrict__ k_inv,
    const float* __restrict__ v_inv, long total, int B, int Hkv, int S_src,
    int S, int Smax, int D) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int d8n = D / 8;
  const int d8 = (int)(i % d8n);
  long t = i / d8n;
  const int s = (int)(t % S);
  t /= S;
  const int h = (int)(t % Hkv);
  const long r = t / Hkv;
  const int row = rows[r];
  if (row < 0 || row >= B || s >= Smax || s >= S_src) return;
  const long so = ((r * Hkv + h) * S_src + s) * (long)D + d8 * 8;
  const long dof = (((long)row * Hkv + h) * Smax + s) * (long)D + d8 * 8;
  const bf16x8 kv = *reinterpret_cast<const bf16x8*>(src_k + so);
  const bf16x8 vv = *reinterpret_cast<const bf16x8*>(src_v + so);
  *reinterpret_cast<u32x2_t*>(dst_k + dof) = fp8_quant8(kv, k_inv[h]);
  *reinterpret_cast<u32x2_t*>(dst_v + dof) = fp8_quant8(vv, v_inv[h]);
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

// One launcher for both decode entry points: FUSED picks the q source and
// the append step.  waves is the block width (4 or 8); workspaces are only
// touched when splits > 1.
template <bool FUSED>
static hipError_t launch_decode_attn(const void* qsrc, void* kc, void* vc,
                                     void* out, const float* cosT,
                                     const float* sinT, const int* seq_lens,
                                     float* ws_o, float* ws_ml, int splits,
                                     int waves, int B, int H, int Hkv,
                                     int Smax, int D, float scale,
                                     hipStream_t stream) {
  if (Hkv < 1 || H < 1 || H % Hkv || Smax < 1 || B < 1 || splits < 1 ||
      (D & 1) || (D != 64 && D != 128) || (waves != 4 && waves != 8))
    return hipErrorInvalidValue;
  const int G = H / Hkv;
  if (G > DEC_MAXG) return hipErrorInvalidValue;
  if (splits > 1 && (!ws_o || !ws_ml)) return hipErrorInvalidValue;
  // sm_o [NW][G][D] | sm_ml [NW][G][2]
  const size_t lds = (size_t)waves * (G * D + 2 * G) * sizeof(float);
  dim3 grid(Hkv, B, splits);
#define DEC_LAUNCH(GV, DV, NWV)                                               \
  hipLaunchKernelGGL((decode_attn_kernel<GV, DV, NWV, FUSED>), grid,          \
                     dim3(NWV * WAVE), lds, stream, (const bf16*)qsrc,        \
                     (bf16*)kc, (bf16*)vc, ws_o, ws_ml, (bf16*)out, cosT,     \
                     sinT, seq_lens, H, Hkv, Smax, scale, splits)
#define DEC_CASE(GV, DV)                                                      \
  case GV * 1000 + DV:                                                        \
    if (waves == 8) DEC_LAUNCH(GV, DV, 8);                                    \
    else DEC_LAUNCH(GV, DV, 4);                                               \
    break;
#define DEC_ALL_G(DV)                                                 \
  DEC_CASE(1, DV) DEC_CASE(2, DV) DEC_CASE(3, DV) DEC_CASE(4, DV)     \
  DEC_CASE(5, DV) DEC_CASE(6, DV) DEC_CASE(7, DV) DEC_CASE(8, DV)
  switch (G * 1000 + D) {
    DEC_ALL_G(64) DEC_ALL_G(128)
    default:
      return hipErrorInvalidValue;
  }
#undef DEC_ALL_G
#undef DEC_CASE
#undef DEC_LAUNCH
  HIP_CHECK_LAUNCH();
  if (splits > 1) {   // splits==1 normalized + wrote out in the decode kernel
    hipLaunchKernelGGL(decode_attn_combine_kernel, dim3(H, B), dim3(128), 0,
                       stream, ws_o, ws_ml, (bf16*)out, H, G, D, splits);
    HIP_CHECK_LAUNCH();
  }
  return hipSuccess;
}

// FP8-cache launcher: the checks, grid, LDS size and combine step of
// launch_decode_attn<true>.
static hipError_t launch_decode_attn_fp8(
    const void* qsrc, void* kc, void* vc, void* out, const float* cosT,
    const float* sinT, const int* seq_lens, const float* k_scale,
    const float* v_scale, const float* k_inv, const float* v_inv, float* ws_o,
    float* ws_ml, int splits, int waves, int B, int H, int Hkv, int Smax,
    int D, float scale, hipStream_t stream) {
  if (Hkv < 1 || H < 1 || H % Hkv || Smax < 1 || B < 1 || splits < 1 ||
      (D != 64 && D != 128) || (waves != 4 && waves != 8))
    return hipErrorInvalidValue;
  if (!k_scale || !v_scale || !k_inv || !v_inv) return hipErrorInvalidValue;
  // the kernel addresses a (b, kv-head) slab with 32-bit byte offsets
  if ((long)Smax * D > 0x7fffffffL) return hipErrorInvalidValue;
  const int G = H / Hkv;
  if (G > DEC_MAXG) return hipErrorInvalidValue;
  if (splits > 1 && (!ws_o || !ws_ml)) return hipErrorInvalidValue;
  const size_t lds = (size_t)waves * (G * D + 2 * G) * sizeof(float);
  dim3 grid(Hkv, B, splits);
#define DEC8_LAUNCH(GV, DV, NWV)                                              \
  hipLaunchKernelGGL(                                                         \
      (decode_attn_fp8_kernel<GV, DV, NWV, Fp8Epl<GV, DV>::value>), grid,     \
                     dim3(NWV * WAVE), lds, stream, (const bf16*)qsrc,        \
                     (unsigned char*)kc, (unsigned char*)vc, ws_o, ws_ml,     \
                     (bf16*)out, cosT, sinT, seq_lens, k_scale, v_scale,      \
                     k_inv, v_inv, H, Hkv, Smax, scale, splits)
#define DEC8_CASE(GV, DV)                                                     \
  case GV * 1000 + DV:                                                        \
    if (waves == 8) DEC8_LAUNCH(GV, DV, 8);                                   \
    else DEC8_LAUNCH(GV, DV, 4);                                              \
    break;
#define DEC8_ALL_G(DV)                                                    \
  DEC8_CASE(1, DV) DEC8_CASE(2, DV) DEC8_CASE(3, DV) DEC8_CASE(4, DV)     \
  DEC8_CASE(5, DV) DEC8_CASE(6, DV) DEC8_CASE(7, DV) DEC8_CASE(8, DV)
  switch (G * 1000 + D) {
    DEC8_ALL_G(64) DEC8_ALL_G(128)
    default:
      return hipErrorInvalidValue;
  }
#undef DEC8_ALL_G
#undef DEC8_CASE
#undef DEC8_LAUNCH
  HIP_CHECK_LAUNCH();
  if (splits > 1) {
    hipLaunchKernelGGL(decode_attn_combine_kernel, dim3(H, B), dim3(128), 0,
                       stream, ws_o, ws_ml, (bf16*)out, H, G, D, splits);
    HIP_CHECK_LAUNCH();
  }
  return hipSuccess;
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
                              float* ws_o, float* ws_ml, int splits, int waves,
                              int B, int H, int Hkv, int Smax, int D,
                              float scale, hipStream_t stream) {
  return launch_decode_attn<false>(q, const_cast<void*>(kc),
                                   const_cast<void*>(vc), out, nullptr,
                                   nullptr, seq_lens, ws_o, ws_ml, splits,
                                   waves, B, H, Hkv, Smax, D, scale, stream);
}

hipError_t sentio_decode_attn_fused(const void* qkv, void* kc, void* vc,
                                    void* out, const float* cosT,
                                    const float* sinT, const int* seq_lens,
                                    float* ws_o, float* ws_ml, int splits,
                                    int waves, int B, int H, int Hkv,
                                    int Smax, int D, float scale,
                                    hipStream_t stream) {
  return launch_decode_attn<true>(qkv, kc, vc, out, cosT, sinT, seq_lens,
                                  ws_o, ws_ml, splits, waves, B, H, Hkv, Smax,
                                  D, scale, stream);
}

hipError_t sentio_decode_attn_fused_fp8(
    const void* qkv, void* kc, void* vc, void* out, const float* cosT,
    const float* sinT, const int* seq_lens, const float* k_scale,
    const float* v_scale, const float* k_inv, const float* v_inv, float* ws_o,
    float* ws_ml, int splits, int waves, int B, int H, int Hkv, int Smax,
    int D, float scale, hipStream_t stream) {
  return launch_decode_attn_fp8(qkv, kc, vc, out, cosT, sinT, seq_lens,
                                k_scale, v_scale, k_inv, v_inv, ws_o, ws_ml,
                                splits, waves, B, H, Hkv, Smax, D, scale,
                                stream);
}

hipError_t sentio_kv_store_fp8(const void* src_k, const void* src_v,
                               void* dst_k, void* dst_v, const int* rows,
                               const float* k_inv, const float* v_inv, int n,
                               int B, int Hkv, int S_src, int S, int Smax,
                               int D, hipStream_t stream) {
  if (n < 0 || B < 1 || Hkv < 1 || S < 0 || S > S_src || S > Smax ||
      D < 8 || (D % 8) || !rows || !k_inv || !v_inv)
    return hipErrorInvalidValue;
  const long total = (long)n * Hkv * S * (D / 8);
  if (total == 0) return hipSuccess;
  const int threads = 256;
  const long blocks = (total + threads - 1) / threads;
  if (blocks > 0x7fffffffL) return hipErrorInvalidValue;
  hipLaunchKernelGGL(kv_store_fp8_kernel, dim3((unsigned)blocks),
                     dim3(threads), 0, stream, (const bf16*)src_k,
                     (const bf16*)src_v, (unsigned char*)dst_k,
                     (unsigned char*)dst_v, rows, k_inv, v_inv, total, B, Hkv,
                     S_src, S, Smax, D);
  HIP_CHECK_LAUNCH();
  return hipSuccess;
}

}  // extern "C"

