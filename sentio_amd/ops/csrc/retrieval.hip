// Retrieval kernels: fused cosine scoring scan over the in-HBM index (K2)
// and BM25 CSR-postings scoring (K3).  Memory-bandwidth-bound by design:
// the cosine scan reads each index row exactly once and amortizes it over
// all B queries of the batch (queries staged in LDS).
#include "common.h"
#include "sentio_kernels.h"

// mat [N, D] f16-or-bf16 row-major (L2-normalized rows), q [B, D] same dtype
// (normalized), scores [B, N] f32.
// Block = 4 waves; queries staged once in LDS; each wave scans rows
// grid-strided, lane l owns elements [l*E, l*E+E) of a row (E = D/64).
// Wave reduces B dots per row via shfl.
// E = D/64 is a template constant so the row cache rv[] stays in registers
// (runtime-indexed ext arrays spill to scratch — guide §5.4 rule 20).
template <typename T, int E>
__global__ void cosine_scores_kernel(const T* __restrict__ mat,
                                     const T* __restrict__ q,
                                     float* __restrict__ scores,
                                     long N, int B) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* qs = reinterpret_cast<float*>(smem);  // [B][D] f32
  constexpr int D = E * WAVE;

  // cooperative query staging
  for (int i = threadIdx.x; i < B * D; i += blockDim.x)
    qs[i] = (float)q[i];
  __syncthreads();

  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x / WAVE;
  const int waves_per_block = blockDim.x / WAVE;
  const long wave_global = (long)blockIdx.x * waves_per_block + wid;
  const long wave_count = (long)gridDim.x * waves_per_block;

  typedef T tvec8 __attribute__((ext_vector_type(8)));
  for (long row = wave_global; row < N; row += wave_count) {
    const T* r = mat + row * (long)D + lane * E;
    float rv[E];
    // vectorized 16-byte row loads (scalar f16/bf16 loads are ~2.5x slower,
    // guide G13); E >= 8 is the hot path (D >= 512)
    if constexpr (E % 8 == 0) {
#pragma unroll
      for (int e8 = 0; e8 < E / 8; ++e8) {
        tvec8 v = *reinterpret_cast<const tvec8*>(r + e8 * 8);
#pragma unroll
        for (int j = 0; j < 8; ++j) rv[e8 * 8 + j] = (float)v[j];
      }
    } else {
#pragma unroll
      for (int e = 0; e < E; ++e) rv[e] = (float)r[e];
    }
    for (int b = 0; b < B; ++b) {
      const float* qb = qs + (long)b * D + lane * E;
      float acc = 0.f;
#pragma unroll
      for (int e = 0; e < E; ++e) acc += rv[e] * qb[e];
      acc = wave_sum(acc);
      if (lane == 0) scores[(long)b * N + row] = acc;
    }
  }
}

template <typename T>
hipError_t launch_cosine(const void* mat, const void* q, float* scores, long N,
                         int D, int B, hipStream_t stream) {
  if (D % WAVE != 0) return hipErrorInvalidValue;
  size_t lds = (size_t)B * D * sizeof(float);
  if (lds > 160 * 1024) return hipErrorInvalidValue;
  long blocks = (N + 3) / 4;
  if (blocks > 4096) blocks = 4096;
  dim3 g((unsigned)blocks), blk(256);
  switch (D / WAVE) {
#define CASE_E(EV)                                                         \
  case EV:                                                                 \
    hipLaunchKernelGGL((cosine_scores_kernel<T, EV>), g, blk, lds, stream, \
                       (const T*)mat, (const T*)q, scores, N, B);          \
    break;
    CASE_E(1) CASE_E(2) CASE_E(4) CASE_E(6) CASE_E(8)
    CASE_E(12) CASE_E(16) CASE_E(24) CASE_E(32)
#undef CASE_E
    default:
      return hipErrorInvalidValue;
  }
  HIP_CHECK_LAUNCH();
  return hipSuccess;
}

// ---------------------------------------------------------------- BM25
// Grid-stride over the query's postings union.  For posting j of term t:
//   contrib = idf[t] * (tf*(k1+1)/(tf + k1*(1-b+b*dl/avgdl)) + delta)
// atomically accumulated into scores[doc].  T (query terms) is small, so a
// linear scan finds the owning term.
__global__ void bm25_kernel(const long* __restrict__ term_ids,
                            const long* __restrict__ qoff,   // [T+1] prefix
                            const long* __restrict__ starts, // [T] indptr[t]
                            const int* __restrict__ post_doc,
                            const float* __restrict__ post_tf,
                            const float* __restrict__ idf,
                            const float* __restrict__ doc_len,
                            float* __restrict__ scores,
                            int T, long total, float k1, float b,
                            float inv_avgdl, float delta) {
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total;
       i += (long)gridDim.x * blockDim.x) {
    int t = 0;
    while (t + 1 < T && i >= qoff[t + 1]) ++t;
    const long p = starts[t] + (i - qoff[t]);
    const int doc = post_doc[p];
    const float tf = post_tf[p];
    const float denom = tf + k1 * (1.f - b + b * doc_len[doc] * inv_avgdl);
    const float contrib =
        idf[term_ids[t]] * (tf * (k1 + 1.f) / denom + delta);
    atomicAdd(&scores[doc], contrib);
  }
}


// ------------------------------------------------------------- fusion (K4)
// Batched device fusion of per-source top-k candidate lists
// (reference hybrid.py:204-259 semantics; host fusion.py is the oracle).
// One block per query; union <= FUSE_MAX entries; ids are int64 (-1 = pad).
// method: 0=rrf, 1=weighted_rrf, 2=comb_sum.
#define FUSE_MAX 128
__global__ void fuse_topk_kernel(
    const long* __restrict__ d_ids, const float* __restrict__ d_scores,
    const long* __restrict__ s_ids, const float* __restrict__ s_scores,
    long* __restrict__ out_ids, float* __restrict__ out_scores,
    int Kd, int Ks, int top_k, int method, float rrf_k, float dw, float sw) {
  __shared__ long ids[FUSE_MAX];
  __shared__ float score[FUSE_MAX];
  __shared__ unsigned char owner[FUSE_MAX];
  __shared__ float red[2];
  const int q = blockIdx.x;
  const int n = Kd + Ks;
  const int t = threadIdx.x;

  // load candidates in insertion order: dense ranks then sparse ranks
  for (int i = t; i < n; i += blockDim.x) {
    ids[i] = (i < Kd) ? d_ids[(long)q * Kd + i] : s_ids[(long)q * Ks + (i - Kd)];
    score[i] = 0.f;
    owner[i] = 0;
  }
  __syncthreads();
  // owner = first slot with this id (stable insertion order)
  for (int i = t; i < n; i += blockDim.x) {
    if (ids[i] < 0) continue;
    int first = i;
    for (int j = 0; j < i; ++j)
      if (ids[j] == ids[i]) { first = j; break; }
    owner[i] = (first == i);
  }
  __syncthreads();

  // per-source normalization constants (comb_sum only)
  float dmin = 0.f, dscale = 0.f, smin = 0.f, sscale = 0.f;
  if (method == 2) {
    if (t == 0) {
      float lo = INFINITY, hi = -INFINITY;
      for (int i = 0; i < Kd; ++i) {
        const long id = d_ids[(long)q * Kd + i];
        if (id < 0) continue;
        const float v = d_scores[(long)q * Kd + i];
        lo = fminf(lo, v); hi = fmaxf(hi, v);
      }
      red[0] = lo; red[1] = hi;
    }
    __syncthreads();
    dmin = red[0]; dscale = red[1] - red[0];
    __syncthreads();
    if (t == 0) {
      float lo = INFINITY, hi = -INFINITY;
      for (int i = 0; i < Ks; ++i) {
        const long id = s_ids[(long)q * Ks + i];
        if (id < 0) continue;
        const float v = s_scores[(long)q * Ks + i];
        lo = fminf(lo, v); hi = fmaxf(hi, v);
      }
      red[0] = lo; red[1] = hi;
    }
    __syncthreads();
    smin = red[0]; sscale = red[1] - red[0];
  }

  // accumulate each entry's contribution into its owner slot
  for (int i = t; i < n; i += blockDim.x) {
    if (ids[i] < 0) continue;
    const bool is_dense = i < Kd;
    const int rank = is_dense ? i : (i - Kd);
    float c;
    if (method == 2) {
      const float raw = is_dense ? d_scores[(long)q * Kd + rank]
                                 : s_scores[(long)q * Ks + rank];
      const float mn = is_dense ? dmin : smin;
      const float sc = is_dense ? dscale : sscale;
      const float norm = (sc > 0.f) ? (raw - mn) / sc : 1.f;
      c = (is_dense ? dw : sw) * norm;
    } else {
      const float w = (method == 0) ? 1.f : (is_dense ? dw : sw);
      c = w / (rrf_k + (float)rank);
    }
    // find owner slot
    int o = i;
    for (int j = 0; j < i; ++j)
      if (ids[j] == ids[i]) { o = j; break; }
    atomicAdd(&score[o], c);
  }
  __syncthreads();

  // top-k selection: thread 0 scans (n <= 128, k <= 20 — trivial)
  if (t == 0) {
    for (int k = 0; k < top_k; ++k) {
      float best = -INFINITY;
      int bi = -1;
      for (int i = 0; i < n; ++i)
        if (owner[i] && score[i] > best) { best = score[i]; bi = i; }
      if (bi < 0) {
        out_ids[(long)q * top_k + k] = -1;
        out_scores[(long)q * top_k + k] = 0.f;
      } else {
        out_ids[(long)q * top_k + k] = ids[bi];
        out_scores[(long)q * top_k + k] = best;
        owner[bi] = 0;
      }
    }
  }
}

// ------------------------------------------- fp8 dense index: scan + top-k
// The opt-in e4m3fn index (index/dense.py): codes uint8 [N, D], one fp32
// scale per row, fp16 queries.  score[b, n] = scales[n] * sum_d q[b, d] *
// float(code[n, d]); top-k by score descending, ties to the lower row.  No
// [B, N] score matrix exists: selection happens inside the scan.
//
// Scan kernel, persistent grid (one 8-wave block per CU, at most
// IDX_MAX_BLOCKS).  A block walks 128-row chunks, chunk = blockIdx.x +
// i * gridDim.x; wave w takes the chunk's 16-row tile w.  Index rows are
// the B operand of mfma_f32_16x16x32_f16 (column = lane & 15), queries the
// A operand, so lane l ends a tile with the scores of queries (l>>4)*4 + r
// (r = 0..3, per 16-query tile) against index row l & 15, and needs one
// scale.  The contraction order is free, so the k axis is permuted for wide
// loads: lane group g = l >> 4 loads the 16 bytes [u*64 + g*16, +16) of its
// row per 64-wide unit u (four lanes cover 64 contiguous bytes; two
// consecutive loads a 128 B line) and feeds bytes 0..7 to MFMA step 2u and
// bytes 8..15 to step 2u+1; a D % 64 == 32 tail is one 8-byte step.  Bytes
// become f16 in registers with v_cvt_scalef32_pk_f16_fp8 at scale 1.0
// (exact: every e4m3fn value is an f16 value), one instruction per two
// codes.  Queries are staged once per block in LDS in that same fragment
// order (step, query tile, lane: one conflict-free 16 B read per MFMA); at
// D = 1024 the 32-query fragments alone would be 256 registers per lane.
// QT (16-query tiles, 1 or 2) is a template constant, so B <= 16 runs half
// the MFMAs and LDS reads.  NU_CT = 16 is D = 1024 with the whole tile in
// registers and the next chunk's loads issued ahead of the MFMAs and the
// selection; NU_CT = 0 is any other D, streamed four units at a time.
//
// Selection.  Per query the block keeps in LDS a list of IDX_CAP (score,
// row) places, its fill count and a threshold (-inf until k candidates
// exist, then the k-th best score so far).  A lane whose score is >= the
// threshold (>=: an equal score with a lower row must still win) appends
// with one LDS atomic.  After every chunk, between two barriers, wave w
// compacts the lists of queries w, w+8, .. that could overflow in the next
// chunk (more than IDX_CAP - 128 entries): every entry's rank under (score
// desc, row asc) is counted against the list, ranks below k move to place
// rank (the list comes out sorted), the threshold becomes the score at
// rank k-1.  A chunk appends at most 128 entries per query and a compacted
// list holds at most k <= 128, so an append never runs past IDX_CAP.  A
// block ends by compacting every list and writing k places per query to
// the workspace [B, blocks, k], (-inf, -1) past the fill count.
//
// Merge kernel, one 1024-thread block per query over its blocks * k
// places: (score, row) packs into one 64-bit key whose unsigned order is
// the result order, an 8-bit radix select finds the k-th key in 8 passes,
// the <= 128 keys at or above it are ranked against each other and written
// in order.
#define IDX_WAVES 8
#define IDX_CHUNK (IDX_WAVES * 16)   // rows per block iteration
#define IDX_CAP 256                  // list places per query
#define IDX_KMAX 128
#define IDX_MAX_BLOCKS 256
#define IDX_MERGE_THREADS 1024
// fp32 VALU work stays on the scalar forms, as in verify_attn_kernel and
// for the reason given there (attention.hip, VER_NO_PK_F32)
#define IDX_NO_PK_F32 __attribute__((target("no-packed-fp32-ops")))

typedef _Float16 f16x2_t __attribute__((ext_vector_type(2)));
typedef _Float16 f16x4_t __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8_t __attribute__((ext_vector_type(8)));
typedef unsigned u32x2_t __attribute__((ext_vector_type(2)));
typedef unsigned u32x4_t __attribute__((ext_vector_type(4)));

// 8 e4m3fn bytes (two dwords, byte j = element j) -> 8 f16, exact
__device__ __forceinline__ f16x8_t idx_cvt8(unsigned lo, unsigned hi) {
  const f16x2_t a = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8((int)lo, 1.f, false);
  const f16x2_t b = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8((int)lo, 1.f, true);
  const f16x2_t c = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8((int)hi, 1.f, false);
  const f16x2_t d = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8((int)hi, 1.f, true);
  const f16x4_t ab = __builtin_shufflevector(a, b, 0, 1, 2, 3);
  const f16x4_t cd = __builtin_shufflevector(c, d, 0, 1, 2, 3);
  return __builtin_shufflevector(ab, cd, 0, 1, 2, 3, 4, 5, 6, 7);
}

// first k index of MFMA step s for lane group g (NU whole 64-wide units)
__device__ __forceinline__ int idx_kbase(int s, int g, int NU) {
  return s < 2 * NU ? (s >> 1) * 64 + g * 16 + (s & 1) * 8 : s * 32 + g * 8;
}

// one MFMA step: 8 codes of this lane's row against QT query tiles; qf is
// the staged fragments already offset by lane * 16
template <int QT>
__device__ __forceinline__ void idx_step(f32x4 (&acc)[QT], const char* qf,
                                         int s, unsigned lo, unsigned hi) {
  const f16x8_t b = idx_cvt8(lo, hi);
#pragma unroll
  for (int t = 0; t < QT; ++t) {
    const f16x8_t a =
        *reinterpret_cast<const f16x8_t*>(qf + (s * QT + t) * (WAVE * 16));
    acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, acc[t], 0, 0, 0);
  }
}

// wave-wide: sort one query's list by (score desc, row asc), keep the best
// k, set the threshold once k exist.  Returns the new fill count.
__device__ __forceinline__ int idx_compact(float* cs, int* cr, int* cnt,
                                           float* thr, int k, int lane) {
  const int n = min(*cnt, IDX_CAP);
  constexpr int PER = IDX_CAP / WAVE;
  float s[PER];
  int r[PER], rank[PER];
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    const int e = lane + i * WAVE;
    s[i] = e < n ? cs[e] : -INFINITY;
    r[i] = e < n ? cr[e] : 0x7fffffff;
    rank[i] = 0;
  }
  for (int j = 0; j < n; ++j) {
    const float sj = cs[j];
    const int rj = cr[j];
#pragma unroll
    for (int i = 0; i < PER; ++i)
      rank[i] += (sj > s[i] || (sj == s[i] && rj < r[i])) ? 1 : 0;
  }
  // every lane's ranks depend on all of the reads above and a wave's LDS
  // operations complete in order: the moves below cannot pass them
  __builtin_amdgcn_wave_barrier();
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    if (lane + i * WAVE < n && rank[i] < k) {
      cs[rank[i]] = s[i];
      cr[rank[i]] = r[i];
      if (rank[i] == k - 1) *thr = s[i];
    }
  }
  const int kept = min(n, k);
  if (lane == 0) *cnt = kept;
  __builtin_amdgcn_wave_barrier();
  return kept;
}

template <int QT, int NU_CT>
__launch_bounds__(IDX_WAVES * WAVE)
IDX_NO_PK_F32 __global__ void index_scan_fp8_kernel(
    const unsigned char* __restrict__ codes, const float* __restrict__ scales,
    const _Float16* __restrict__ q, float* __restrict__ ws_s,
    int* __restrict__ ws_r, long N, int D, int Bg, int k, int qbase) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int NS = D / 32;                       // MFMA steps of a row
  const int NU = NU_CT ? NU_CT : D / 64;       // whole 64-wide units
  char* qfrag = smem;                          // [NS][QT][64 lanes] x 16 B
  float* cand_s = reinterpret_cast<float*>(smem + (size_t)NS * QT * WAVE * 16);
  int* cand_r = reinterpret_cast<int*>(cand_s + QT * 16 * IDX_CAP);
  int* cnt = cand_r + QT * 16 * IDX_CAP;       // [QT*16]
  float* thr = reinterpret_cast<float*>(cnt + QT * 16);

  const int tid = threadIdx.x;
  const int lane = tid & (WAVE - 1);
  const int w = tid / WAVE;
  const int c = lane & 15, g = lane >> 4;

  for (int i = tid; i < NS * QT * WAVE; i += IDX_WAVES * WAVE) {
    const int l = i & (WAVE - 1);
    const int t = (i / WAVE) % QT, s = (i / WAVE) / QT;
    const int qi = t * 16 + (l & 15);
    u32x4_t v = {0u, 0u, 0u, 0u};
    if (qi < Bg)
      v = *reinterpret_cast<const u32x4_t*>(q + (long)qi * D +
                                            idx_kbase(s, l >> 4, NU));
    *reinterpret_cast<u32x4_t*>(qfrag + (long)i * 16) = v;
  }
  if (tid < QT * 16) {
    cnt[tid] = 0;
    thr[tid] = -INFINITY;
  }
  __syncthreads();

  const char* qf = qfrag + lane * 16;
  const long nchunks = (N + IDX_CHUNK - 1) / IDX_CHUNK;
  // this lane's row of a chunk, clamped: rows at or past N load row N-1 and
  // are dropped at the append
  // (both lambdas must inline: a call would put acc and the captures in
  // scratch)
  auto row_ptr = [&](long chunk) __attribute__((always_inline)) {
    long row = chunk * IDX_CHUNK + w * 16 + c;
    if (row > N - 1) row = N - 1;
    return codes + row * (long)D;
  };
  // scale, append, then compact what the next chunk could overflow
  auto finish = [&](long chunk, const f32x4 (&acc)[QT])
                    __attribute__((always_inline)) {
    const long row = chunk * IDX_CHUNK + w * 16 + c;
    const bool ok = row < N;
    const float sc = scales[ok ? row : N - 1];
#pragma unroll
    for (int t = 0; t < QT; ++t) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int qi = t * 16 + g * 4 + r;
        const float s = acc[t][r] * sc;
        if (ok && qi < Bg && s >= thr[qi]) {
          const int pos = atomicAdd(&cnt[qi], 1);
          if (pos < IDX_CAP) {
            cand_s[qi * IDX_CAP + pos] = s;
            cand_r[qi * IDX_CAP + pos] = (int)row;
          }
        }
      }
    }
    __syncthreads();
    for (int qi = w; qi < Bg; qi += IDX_WAVES)
      if (cnt[qi] > IDX_CAP - IDX_CHUNK)
        idx_compact(cand_s + qi * IDX_CAP, cand_r + qi * IDX_CAP, cnt + qi,
                    thr + qi, k, lane);
    __syncthreads();
  };

  if constexpr (NU_CT > 0) {
    u32x4_t cur[NU_CT];
    if ((long)blockIdx.x < nchunks) {
      const unsigned char* rp = row_ptr(blockIdx.x) + g * 16;
#pragma unroll
      for (int u = 0; u < NU_CT; ++u)
        cur[u] = __builtin_nontemporal_load(
            reinterpret_cast<const u32x4_t*>(rp + u * 64));
    }
    for (long chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
      u32x4_t nxt[NU_CT];
#pragma unroll
      for (int u = 0; u < NU_CT; ++u) nxt[u] = cur[u];
      if (chunk + gridDim.x < nchunks) {
        const unsigned char* rp = row_ptr(chunk + gridDim.x) + g * 16;
#pragma unroll
        for (int u = 0; u < NU_CT; ++u)
          nxt[u] = __builtin_nontemporal_load(
              reinterpret_cast<const u32x4_t*>(rp + u * 64));
      }
      f32x4 acc[QT];
#pragma unroll
      for (int t = 0; t < QT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int u = 0; u < NU_CT; ++u) {
        idx_step<QT>(acc, qf, 2 * u, cur[u].x, cur[u].y);
        idx_step<QT>(acc, qf, 2 * u + 1, cur[u].z, cur[u].w);
      }
      finish(chunk, acc);
#pragma unroll
      for (int u = 0; u < NU_CT; ++u) cur[u] = nxt[u];
    }
  } else {
    for (long chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
      const unsigned char* rb = row_ptr(chunk);
      f32x4 acc[QT];
#pragma unroll
      for (int t = 0; t < QT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
      for (int u0 = 0; u0 < NU; u0 += 4) {
        u32x4_t raw[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          raw[i] = u32x4_t{0u, 0u, 0u, 0u};
          if (u0 + i < NU)
            raw[i] = __builtin_nontemporal_load(
                reinterpret_cast<const u32x4_t*>(rb + (u0 + i) * 64 + g * 16));
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          if (u0 + i < NU) {
            idx_step<QT>(acc, qf, 2 * (u0 + i), raw[i].x, raw[i].y);
            idx_step<QT>(acc, qf, 2 * (u0 + i) + 1, raw[i].z, raw[i].w);
          }
        }
      }
      if (D & 32) {
        const u32x2_t tl = __builtin_nontemporal_load(
            reinterpret_cast<const u32x2_t*>(rb + (NS - 1) * 32 + g * 8));
        idx_step<QT>(acc, qf, NS - 1, tl.x, tl.y);
      }
      finish(chunk, acc);
    }
  }

  for (int qi = w; qi < Bg; qi += IDX_WAVES) {
    float* cs = cand_s + qi * IDX_CAP;
    int* cr = cand_r + qi * IDX_CAP;
    const int n = idx_compact(cs, cr, cnt + qi, thr + qi, k, lane);
    const long base = ((long)(qbase + qi) * gridDim.x + blockIdx.x) * k;
    for (int i = lane; i < k; i += WAVE) {
      ws_s[base + i] = i < n ? cs[i] : -INFINITY;
      ws_r[base + i] = i < n ? cr[i] : -1;
    }
  }
}

// (score, row) -> key: larger key = earlier in the result.  Row -1 (an empty
// place) never enters: the merge skips it.
__device__ __forceinline__ unsigned long long idx_key(float s, int r) {
  unsigned u = __float_as_uint(s);
  u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return ((unsigned long long)u << 32) | (unsigned)~r;
}

// wave-uniform call: one LDS atomic per distinct digit in the wave (the top
// bytes of the keys of one query are nearly all equal)
__device__ __forceinline__ void idx_hist_add(int* hist, bool on, int digit,
                                             int lane) {
  unsigned long long todo = __ballot(on);
  while (todo) {
    const int leader = __ffsll((long long)todo) - 1;
    const int d0 = __shfl(digit, leader, WAVE);
    const unsigned long long same = __ballot(on && digit == d0);
    if (lane == leader) atomicAdd(&hist[d0], (int)__popcll(same));
    todo &= ~same;
  }
}

__launch_bounds__(IDX_MERGE_THREADS)
IDX_NO_PK_F32 __global__ void index_merge_kernel(
    const float* __restrict__ ws_s, const int* __restrict__ ws_r,
    float* __restrict__ out_s, long* __restrict__ out_r, int n, int k) {
  __shared__ int hist[256];
  __shared__ unsigned long long sel[IDX_KMAX];
  __shared__ int sh_valid, sh_nsel, sh_digit, sh_want;
  const float* cs = ws_s + (long)blockIdx.x * n;
  const int* cr = ws_r + (long)blockIdx.x * n;
  float* os = out_s + (long)blockIdx.x * k;
  long* orow = out_r + (long)blockIdx.x * k;
  const int tid = threadIdx.x;
  const int lane = tid & (WAVE - 1);

  if (tid == 0) {
    sh_valid = 0;
    sh_nsel = 0;
  }
  __syncthreads();
  int v = 0;
  for (int i = tid; i < n; i += IDX_MERGE_THREADS) v += cr[i] >= 0 ? 1 : 0;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, WAVE);
  if (lane == 0 && v) atomicAdd(&sh_valid, v);
  __syncthreads();
  const int kk = min(k, sh_valid);

  if (kk > 0) {
    // radix select of the kk-th largest key, one byte per pass from the top
    unsigned long long prefix = 0, mask = 0;
    int want = kk;
    for (int shift = 56; shift >= 0; shift -= 8) {
      if (tid < 256) hist[tid] = 0;
      __syncthreads();
      for (int i0 = 0; i0 < n; i0 += IDX_MERGE_THREADS) {
        const int i = i0 + tid;
        const int r = i < n ? cr[i] : -1;
        const unsigned long long key = r >= 0 ? idx_key(cs[i], r) : 0;
        idx_hist_add(hist, r >= 0 && (key & mask) == prefix,
                     (int)((key >> shift) & 255), lane);
      }
      __syncthreads();
      if (tid < WAVE) {
        // lane l owns digits 4l .. 4l+3; above = keys in higher lanes' digits
        int cbin[4];
        int sum = 0;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          cbin[b] = hist[4 * lane + b];
          sum += cbin[b];
        }
        int suf = sum;
        for (int off = 1; off < WAVE; off <<= 1) {
          const int o = __shfl_down(suf, off, WAVE);
          if (lane + off < WAVE) suf += o;
        }
        int above = suf - sum;
#pragma unroll
        for (int b = 3; b >= 0; --b) {
          if (above < want && want <= above + cbin[b]) {
            sh_digit = 4 * lane + b;
            sh_want = want - above;
          }
          above += cbin[b];
        }
      }
      __syncthreads();
      prefix |= (unsigned long long)sh_digit << shift;
      mask |= 255ull << shift;
      want = sh_want;
    }
    // keys are distinct (rows are), so exactly kk keys are >= the kk-th
    for (int i = tid; i < n; i += IDX_MERGE_THREADS) {
      const int r = cr[i];
      if (r < 0) continue;
      const unsigned long long key = idx_key(cs[i], r);
      if (key >= prefix) {
        const int p = atomicAdd(&sh_nsel, 1);
        if (p < IDX_KMAX) sel[p] = key;
      }
    }
    __syncthreads();
    if (tid < kk) {
      const unsigned long long me = sel[tid];
      int rank = 0;
      for (int j = 0; j < kk; ++j) rank += sel[j] > me ? 1 : 0;
      unsigned u = (unsigned)(me >> 32);
      u = (u & 0x80000000u) ? (u & 0x7fffffffu) : ~u;
      os[rank] = __uint_as_float(u);
      orow[rank] = (long)(int)~(unsigned)me;
    }
  }
  for (int i = kk + tid; i < k; i += IDX_MERGE_THREADS) {
    os[i] = -INFINITY;
    orow[i] = -1;
  }
}

template <int QT, int NU_CT>
static hipError_t launch_index_scan(const void* q, const void* codes,
                                    const float* scales, float* ws_s,
                                    int* ws_r, long N, int D, int Bg, int k,
                                    int qbase, int blocks,
                                    hipStream_t stream) {
  const size_t lds = (size_t)(D / 32) * QT * WAVE * 16 +
                     (size_t)QT * 16 * (IDX_CAP * 8 + 8);
  auto kern = index_scan_fp8_kernel<QT, NU_CT>;
  hipError_t e = hipFuncSetAttribute(
      reinterpret_cast<const void*>(kern),
      hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(IDX_WAVES * WAVE), lds,
                     stream, (const unsigned char*)codes, scales,
                     (const _Float16*)q, ws_s, ws_r, N, D, Bg, k, qbase);
  HIP_CHECK_LAUNCH();
  return hipSuccess;
}

// ------------------------------------- masked scan: exact filtered search
// index_scan_masked_kernel is the scan above with a row filter and a second
// element type.  allow is int32 [M, W], M == 1 (one mask for every query) or
// M == B; row n is bit n & 31 of word n >> 5 and W = 4 * chunks, so the bits
// of a 128-row chunk are one aligned 16-byte group per mask.  Bits at or
// past N are cleared as the words are read.  A row whose bit is clear never
// appends, so the lists, the compaction, the overflow bound (a chunk still
// appends at most 128 entries per query), the workspace and the merge are
// those of the unmasked scan.
//
// A filter lets the scan read less.  A block's chunks are taken 64 at a
// time (a window).  The block first ORs the groups of the window's chunks
// over its queries (lane = chunk, wave = query subset, one ballot per wave
// ORed into two LDS words) and every wave reads that 64-bit map after one
// barrier: a chunk with no bit set costs the block nothing further, no
// loads, no MFMAs and no barriers, and every wave walks the same map.  The
// per-query words of the live chunk after the current one (one 16-byte
// load by each of the first M threads) go to a ring of LDS slots before the
// two barriers that end the current chunk, so staging adds no barrier.  The
// append reads the bit of (query, row) from the slot; a wave ORs the slot's
// words over the queries and, if its 16-row tile has no bit set, issues no
// row loads and no MFMAs and appends nothing (wave-uniform).
//
// ET = unsigned char is the e4m3fn index (idx_cvt8, a scale per row).  ET =
// _Float16 is the default index: a 16-byte load is 8 consecutive halves,
// one B operand of mfma_f32_16x16x32_f16 as it stands, and the score is the
// fp32 sum of the fp16 products.  Its query fragments are staged in that
// order (step s, lane group g: k = s*32 + g*8).  Both stream 64-byte units,
// four loads at a time; NU_CT = 16 (e4m3fn, D = 1024) keeps the tile in
// registers and issues the next live chunk's loads ahead of the MFMAs.
// That prefetch is predicated on the next chunk's words, so this variant
// stages two live chunks ahead in a ring of three slots.  A 2048-byte fp16
// row does not fit in registers twice, so fp16 always streams.
template <int QT>
__device__ __forceinline__ void idx_step16(f32x4 (&acc)[QT], const char* qf,
                                           int s, u32x4_t raw) {
  const f16x8_t b = __builtin_bit_cast(f16x8_t, raw);
#pragma unroll
  for (int t = 0; t < QT; ++t) {
    const f16x8_t a =
        *reinterpret_cast<const f16x8_t*>(qf + (s * QT + t) * (WAVE * 16));
    acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, acc[t], 0, 0, 0);
  }
}

// the 16-byte group of one mask row for one chunk, bits at or past N cleared
__device__ __forceinline__ u32x4_t idx_mask_group(const unsigned* allow_row,
                                                  long chunk, long N) {
  u32x4_t v = *reinterpret_cast<const u32x4_t*>(allow_row + chunk * 4);
  const long left = N - chunk * IDX_CHUNK;      // >= 1 for a chunk of the scan
  if (left < IDX_CHUNK) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const long nv = left - 32 * j;
      v[j] &= nv >= 32 ? 0xffffffffu : nv <= 0 ? 0u : (1u << nv) - 1u;
    }
  }
  return v;
}

template <typename ET, int QT, int NU_CT>
__launch_bounds__(IDX_WAVES * WAVE)
IDX_NO_PK_F32 __global__ void index_scan_masked_kernel(
    const ET* __restrict__ rows, const float* __restrict__ scales,
    const _Float16* __restrict__ q, const unsigned* __restrict__ allow,
    int MQ, float* __restrict__ ws_s, int* __restrict__ ws_r, long N, int D,
    int Bg, int k, int qbase) {
  constexpr bool F16 = sizeof(ET) == 2;
  static_assert(!(F16 && NU_CT), "fp16 rows are streamed");
  constexpr int NSLOT = NU_CT ? 3 : 2;         // mask slots in the ring
  constexpr int MWS = QT * 16 * 4;             // words of a slot
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int NS = D / 32;                       // MFMA steps of a row
  const int NU = NU_CT ? NU_CT : (F16 ? D / 32 : D / 64);   // 64-byte units
  char* qfrag = smem;                          // [NS][QT][64 lanes] x 16 B
  float* cand_s = reinterpret_cast<float*>(smem + (size_t)NS * QT * WAVE * 16);
  int* cand_r = reinterpret_cast<int*>(cand_s + QT * 16 * IDX_CAP);
  int* cnt = cand_r + QT * 16 * IDX_CAP;       // [QT*16]
  float* thr = reinterpret_cast<float*>(cnt + QT * 16);
  unsigned* mw = reinterpret_cast<unsigned*>(thr + QT * 16);  // [NSLOT][MWS]
  unsigned* live = mw + NSLOT * MWS;           // [2 windows][2 words]

  const int tid = threadIdx.x;
  const int lane = tid & (WAVE - 1);
  const int w = tid / WAVE;
  const int c = lane & 15, g = lane >> 4;

  for (int i = tid; i < NS * QT * WAVE; i += IDX_WAVES * WAVE) {
    const int l = i & (WAVE - 1);
    const int t = (i / WAVE) % QT, s = (i / WAVE) / QT;
    const int qi = t * 16 + (l & 15);
    u32x4_t v = {0u, 0u, 0u, 0u};
    if (qi < Bg)
      v = *reinterpret_cast<const u32x4_t*>(
          q + (long)qi * D + idx_kbase(s, l >> 4, F16 ? 0 : NU));
    *reinterpret_cast<u32x4_t*>(qfrag + (long)i * 16) = v;
  }
  if (tid < QT * 16) {
    cnt[tid] = 0;
    thr[tid] = -INFINITY;
  }
  if (tid < 4) live[tid] = 0;
  __syncthreads();

  const char* qf = qfrag + lane * 16;
  const long nchunks = (N + IDX_CHUNK - 1) / IDX_CHUNK;
  const long W = nchunks * 4;
  const long first = blockIdx.x, grid = gridDim.x;
  // this wave's 16 bits of a chunk: word w >> 1, upper or lower half
  const int mword = w >> 1, mshift = (w & 1) * 16;
  // (the lambdas must inline: a call would put acc and the captures in
  // scratch)
  auto row_ptr = [&](long chunk) __attribute__((always_inline)) {
    long row = chunk * IDX_CHUNK + w * 16 + c;
    if (row > N - 1) row = N - 1;              // its bit is clear
    return reinterpret_cast<const char*>(rows + row * (long)D) + g * 16;
  };
  // does any query of the block allow a row of this wave's tile?  Lanes past
  // the staged queries read query 0 again
  auto tile_live = [&](int slot) __attribute__((always_inline)) {
    const unsigned wd = mw[slot * MWS + (lane < MQ ? lane : 0) * 4 + mword];
    return __ballot(((wd >> mshift) & 0xffffu) != 0u) != 0ull;
  };
  auto stage_load = [&](long chunk) __attribute__((always_inline)) {
    u32x4_t v = {0u, 0u, 0u, 0u};
    if (tid < MQ) v = idx_mask_group(allow + (long)tid * W, chunk, N);
    return v;
  };
  auto stage_store = [&](int slot, u32x4_t v) __attribute__((always_inline)) {
    if (tid < MQ) *reinterpret_cast<u32x4_t*>(mw + slot * MWS + tid * 4) = v;
  };
  // scale and append the allowed rows, publish the staged words, then
  // compact what the next chunk could overflow
  auto finish = [&](long chunk, int slot, bool on, const f32x4 (&acc)[QT],
                    bool stage, int sslot, u32x4_t sv)
                    __attribute__((always_inline)) {
    if (on) {
      const long row = chunk * IDX_CHUNK + w * 16 + c;
      float sc = 1.f;
      if constexpr (!F16) sc = scales[row < N ? row : N - 1];
      const unsigned* mq = mw + slot * MWS + mword;
#pragma unroll
      for (int t = 0; t < QT; ++t) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int qi = t * 16 + g * 4 + r;
          const float s = F16 ? acc[t][r] : acc[t][r] * sc;
          const unsigned bit = (mq[(MQ == 1 ? 0 : qi) * 4] >> (mshift + c)) & 1u;
          if (qi < Bg && bit && s >= thr[qi]) {
            const int pos = atomicAdd(&cnt[qi], 1);
            if (pos < IDX_CAP) {
              cand_s[qi * IDX_CAP + pos] = s;
              cand_r[qi * IDX_CAP + pos] = (int)row;
            }
          }
        }
      }
    }
    if (stage) stage_store(sslot, sv);
    __syncthreads();
    for (int qi = w; qi < Bg; qi += IDX_WAVES)
      if (cnt[qi] > IDX_CAP - IDX_CHUNK)
        idx_compact(cand_s + qi * IDX_CAP, cand_r + qi * IDX_CAP, cnt + qi,
                    thr + qi, k, lane);
    __syncthreads();
  };
  // 16 bytes of a unit -> its MFMA steps
  auto unit = [&](f32x4 (&acc)[QT], int u, u32x4_t raw)
                  __attribute__((always_inline)) {
    if constexpr (F16) {
      idx_step16<QT>(acc, qf, u, raw);
    } else {
      idx_step<QT>(acc, qf, 2 * u, raw.x, raw.y);
      idx_step<QT>(acc, qf, 2 * u + 1, raw.z, raw.w);
    }
  };

  u32x4_t cur[NU_CT ? NU_CT : 1];
#pragma unroll
  for (int u = 0; u < (NU_CT ? NU_CT : 1); ++u) cur[u] = u32x4_t{0u, 0u, 0u, 0u};

  int par = 0;
  for (long it0 = 0; first + it0 * grid < nchunks; it0 += 64, par ^= 1) {
    // the window's live map: lane = chunk, wave = queries w, w + 8, ..
    {
      const long ch = first + (it0 + lane) * grid;
      unsigned any = 0u;
      if (ch < nchunks)
        for (int m = w; m < MQ; m += IDX_WAVES) {
          const u32x4_t v = idx_mask_group(allow + (long)m * W, ch, N);
          any |= v.x | v.y | v.z | v.w;
        }
      const unsigned long long bal = __ballot(any != 0u);
      if (lane == 0 && bal) {
        atomicOr(&live[par * 2], (unsigned)bal);
        atomicOr(&live[par * 2 + 1], (unsigned)(bal >> 32));
      }
    }
    __syncthreads();
    unsigned long long lv =
        (unsigned long long)__builtin_amdgcn_readfirstlane(live[par * 2]) |
        ((unsigned long long)__builtin_amdgcn_readfirstlane(live[par * 2 + 1])
         << 32);
    if (tid < 2) live[(par ^ 1) * 2 + tid] = 0u;   // the next window's words
    {
      unsigned long long t = lv;                 // the first NSLOT - 1 chunks
#pragma unroll
      for (int s = 0; s < NSLOT - 1; ++s) {
        if (t) {
          const int l = __ffsll((long long)t) - 1;
          t &= t - 1;
          stage_store(s, stage_load(first + (it0 + l) * grid));
        }
      }
    }
    __syncthreads();

    int slot = 0;
    bool cur_on = false;
    if constexpr (NU_CT > 0) {
      if (lv) {
        const int l = __ffsll((long long)lv) - 1;
        cur_on = tile_live(0);
        if (cur_on) {
          const char* rp = row_ptr(first + (it0 + l) * grid);
#pragma unroll
          for (int u = 0; u < NU_CT; ++u)
            cur[u] = __builtin_nontemporal_load(
                reinterpret_cast<const u32x4_t*>(rp + u * 64));
        }
      }
    }
    while (lv) {
      const long chunk = first + (it0 + __ffsll((long long)lv) - 1) * grid;
      lv &= lv - 1;
      // the live chunk whose words this iteration stages: the next one, or
      // the one after it where the next one's are already needed here
      unsigned long long ah = lv;
      if (NU_CT) ah &= ah - 1;
      const bool stage = ah != 0ull;
      const int sslot = (slot + NSLOT - 1) % NSLOT;
      u32x4_t sv = {0u, 0u, 0u, 0u};
      if (stage)
        sv = stage_load(first + (it0 + __ffsll((long long)ah) - 1) * grid);
      f32x4 acc[QT];
#pragma unroll
      for (int t = 0; t < QT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};

      if constexpr (NU_CT > 0) {
        u32x4_t nxt[NU_CT];
#pragma unroll
        for (int u = 0; u < NU_CT; ++u) nxt[u] = cur[u];
        bool nxt_on = false;
        if (lv) {
          nxt_on = tile_live((slot + 1) % NSLOT);
          if (nxt_on) {
            const char* rp =
                row_ptr(first + (it0 + __ffsll((long long)lv) - 1) * grid);
#pragma unroll
            for (int u = 0; u < NU_CT; ++u)
              nxt[u] = __builtin_nontemporal_load(
                  reinterpret_cast<const u32x4_t*>(rp + u * 64));
          }
        }
        if (cur_on) {
#pragma unroll
          for (int u = 0; u < NU_CT; ++u) unit(acc, u, cur[u]);
        }
        finish(chunk, slot, cur_on, acc, stage, sslot, sv);
#pragma unroll
        for (int u = 0; u < NU_CT; ++u) cur[u] = nxt[u];
        cur_on = nxt_on;
      } else {
        const bool on = tile_live(slot);
        if (on) {
          const char* rb = row_ptr(chunk);
          for (int u0 = 0; u0 < NU; u0 += 4) {
            u32x4_t raw[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              raw[i] = u32x4_t{0u, 0u, 0u, 0u};
              if (u0 + i < NU)
                raw[i] = __builtin_nontemporal_load(
                    reinterpret_cast<const u32x4_t*>(rb + (u0 + i) * 64));
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
              if (u0 + i < NU) unit(acc, u0 + i, raw[i]);
          }
          if constexpr (!F16) {
            if (D & 32) {
              const u32x2_t tl = __builtin_nontemporal_load(
                  reinterpret_cast<const u32x2_t*>(rb - g * 16 + (NS - 1) * 32 +
                                                   g * 8));
              idx_step<QT>(acc, qf, NS - 1, tl.x, tl.y);
            }
          }
        }
        finish(chunk, slot, on, acc, stage, sslot, sv);
      }
      slot = (slot + 1) % NSLOT;
    }
  }

  for (int qi = w; qi < Bg; qi += IDX_WAVES) {
    float* cs = cand_s + qi * IDX_CAP;
    int* cr = cand_r + qi * IDX_CAP;
    const int n = idx_compact(cs, cr, cnt + qi, thr + qi, k, lane);
    const long base = ((long)(qbase + qi) * gridDim.x + blockIdx.x) * k;
    for (int i = lane; i < k; i += WAVE) {
      ws_s[base + i] = i < n ? cs[i] : -INFINITY;
      ws_r[base + i] = i < n ? cr[i] : -1;
    }
  }
}

template <typename ET, int QT, int NU_CT>
static hipError_t launch_index_scan_masked(const void* q, const void* rows,
                                           const float* scales,
                                           const int* allow, int MQ,
                                           float* ws_s, int* ws_r, long N,
                                           int D, int Bg, int k, int qbase,
                                           int blocks, hipStream_t stream) {
  const size_t lds = (size_t)(D / 32) * QT * WAVE * 16 +
                     (size_t)QT * 16 * (IDX_CAP * 8 + 8) +
                     (size_t)(NU_CT ? 3 : 2) * QT * 16 * 16 + 16;
  auto kern = index_scan_masked_kernel<ET, QT, NU_CT>;
  hipError_t e = hipFuncSetAttribute(
      reinterpret_cast<const void*>(kern),
      hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(IDX_WAVES * WAVE), lds,
                     stream, (const ET*)rows, scales, (const _Float16*)q,
                     (const unsigned*)allow, MQ, ws_s, ws_r, N, D, Bg, k,
                     qbase);
  HIP_CHECK_LAUNCH();
  return hipSuccess;
}

// --------------------------------- BM25: tiled scoring with fused top-k
// bm25_topk_kernel scores a batch of queries against the CSR postings and
// selects inside the scan: no [B, N] or [N] score array exists in global
// memory.  It rests on two invariants of the index (BM25Index.
// build_tokenized): the postings of a term are sorted by document, and a
// document occurs at most once in a term's list.
//
// The corpus is cut into tiles of BM_TILE consecutive documents; a
// persistent grid (one 8-wave block per CU, at most IDX_MAX_BLOCKS, at most
// one per tile) walks tiles blockIdx.x + i * gridDim.x.  Per tile:
//   1. nd[d] = k1 * (1 - b + b * doc_len[d] / avgdl) goes to LDS once for
//      all queries.
//   2. One lane per (query term, bound) finds by binary search on post_doc,
//      inside [indptr[t], indptr[t+1]), the first posting at or past the
//      tile's first document and the first past its last: every chain of
//      dependent loads of the tile runs in this one pass.  In the same pass
//      wave w ORs the tile's words of masks w, w + 8, ..  A query is live in
//      the tile if one of its terms has a posting there and its mask a bit.
//   3. Per live query the block zeroes an fp32 accumulator tile in LDS, then
//      term by term, in query order, strides over the term's slice with a
//      plain LDS read-add-write of idf * (tf * (k1 + 1) / (tf + nd) + delta),
//      a block barrier after each term.  Within a term every posting is
//      another document, so no two lanes meet: no atomics touch a score, the
//      sum runs in query-term order, and a score is a pure function of the
//      index and the query, whatever the tiling.  A term repeated in a query
//      is added once per occurrence.
//   4. Thread t owns documents 8t .. 8t+7 of the tile (one byte of a mask
//      word: the word load serves 32 documents).  A document whose score is
//      > 0, whose bit is set and whose score is >= the query's threshold is
//      appended to the query's list, the lists / thresholds / idx_compact of
//      the dense scan.  A tile can hold more candidates than a list has
//      places (a term in every document gives BM_TILE), so an append that
//      finds the list full stays pending: the block agrees on that with one
//      __syncthreads_or, wave 0 compacts the list (which frees at least
//      IDX_CAP - k places and raises the threshold) and the pending
//      documents are tested again.  Nothing is ever written past a list and
//      nothing that belongs to the top k is dropped.  The list is also
//      compacted once an append passes (IDX_CAP + k) / 2, which sets the
//      threshold early.
// A block ends as the dense scan does, k places per query to the workspace
// [B, blocks, k], and index_merge_kernel finishes.
#define BM_TILE 4096                 // documents per tile (8 per thread)
#define BM_MAX_TERMS 1024            // query terms per launch
#define BM_THREADS (IDX_WAVES * WAVE)
static_assert(BM_TILE == 8 * BM_THREADS, "thread t owns documents 8t .. 8t+7");

__launch_bounds__(BM_THREADS)
IDX_NO_PK_F32 __global__ void bm25_topk_kernel(
    const long* __restrict__ tids, const int* __restrict__ qoff,
    const long* __restrict__ indptr, const int* __restrict__ post_doc,
    const float* __restrict__ post_tf, const float* __restrict__ idf,
    const float* __restrict__ doc_len, const unsigned* __restrict__ allow,
    int MQ, float* __restrict__ ws_s, int* __restrict__ ws_r, long N,
    long n_terms, int Bg, int TT, int k, float k1, float b, float inv_avgdl,
    float delta) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* nd = reinterpret_cast<float*>(smem);              // [BM_TILE]
  float* acc = nd + BM_TILE;                               // [BM_TILE]
  long* sl = reinterpret_cast<long*>(acc + BM_TILE);       // [TT][2] slice
  float* tidf = reinterpret_cast<float*>(sl + 2 * BM_MAX_TERMS);  // [TT]
  float* cand_s = tidf + BM_MAX_TERMS;                     // [Bg][IDX_CAP]
  int* cand_r = reinterpret_cast<int*>(cand_s + Bg * IDX_CAP);
  int* cnt = cand_r + Bg * IDX_CAP;                        // [32]
  float* thr = reinterpret_cast<float*>(cnt + 32);         // [32]
  int* qo = reinterpret_cast<int*>(thr + 32);              // [33]
  int* mlive = qo + 33;                                    // [32] per mask
  int* qlive = mlive + 32;                                 // [32] per query

  const int tid = threadIdx.x;
  const int lane = tid & (WAVE - 1);
  const int w = tid / WAVE;
  const long W = 4 * ((N + IDX_CHUNK - 1) / IDX_CHUNK);    // words of a mask
  const long ntiles = (N + BM_TILE - 1) / BM_TILE;
  const float k1p1 = k1 + 1.f;
  const int lim = (IDX_CAP + k) / 2;

  // a term id outside the vocabulary has no postings and no weight
  for (int j = tid; j < TT; j += BM_THREADS) {
    const long t = tids[j];
    tidf[j] = (t >= 0 && t < n_terms) ? idf[t] : 0.f;
  }
  if (tid < 32) {
    cnt[tid] = 0;
    thr[tid] = -INFINITY;
  }
  if (tid <= Bg) qo[tid] = qoff[tid];
  __syncthreads();

  for (long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const long d0 = tile * BM_TILE;
    // 1. length norms
#pragma unroll
    for (int i = 0; i < BM_TILE / BM_THREADS; ++i) {
      const int d = tid + i * BM_THREADS;
      nd[d] = d0 + d < N
                  ? k1 * (1.f - b + b * doc_len[d0 + d] * inv_avgdl) : 0.f;
    }
    // 2. slices: lane = (term, bound)
    for (int i = tid; i < 2 * TT; i += BM_THREADS) {
      const long t = tids[i >> 1];
      long lo = 0, hi = 0;
      if (t >= 0 && t < n_terms) {
        lo = indptr[t];
        hi = indptr[t + 1];
      }
      const long target = d0 + (i & 1) * BM_TILE;
      while (lo < hi) {
        const long mid = (lo + hi) >> 1;
        if ((long)post_doc[mid] < target) lo = mid + 1; else hi = mid;
      }
      sl[i] = lo;
    }
    // the tile's words of each mask: 128 words, two per lane
    if (allow == nullptr) {
      if (tid == 0) mlive[0] = 1;
    } else {
      for (int m = w; m < MQ; m += IDX_WAVES) {
        const long w0 = tile * (BM_TILE / 32) + lane;
        unsigned any = 0u;
        if (w0 < W) any |= allow[(long)m * W + w0];
        if (w0 + WAVE < W) any |= allow[(long)m * W + w0 + WAVE];
        const unsigned long long bal = __ballot(any != 0u);
        if (lane == 0) mlive[m] = bal != 0ull;
      }
    }
    __syncthreads();
    if (tid < Bg) {
      int any = 0;
      for (int j = qo[tid]; j < qo[tid + 1]; ++j)
        any |= sl[2 * j + 1] > sl[2 * j] ? 1 : 0;
      qlive[tid] = any & mlive[MQ > 1 ? tid : 0];
    }
    __syncthreads();

    for (int q = 0; q < Bg; ++q) {
      if (!qlive[q]) continue;                   // block-uniform
      // 3. scores of the tile for query q
      f32x4* mine = reinterpret_cast<f32x4*>(acc) + 2 * tid;
      mine[0] = f32x4{0.f, 0.f, 0.f, 0.f};
      mine[1] = f32x4{0.f, 0.f, 0.f, 0.f};
      __syncthreads();
      for (int j = qo[q]; j < qo[q + 1]; ++j) {
        const long hi = sl[2 * j + 1];
        const float wj = tidf[j];
        for (long p = sl[2 * j] + tid; p < hi; p += BM_THREADS) {
          const unsigned d = (unsigned)((long)post_doc[p] - d0);
          const float tf = post_tf[p];
          if (d < BM_TILE)                       // holds for sorted postings
            acc[d] += wj * (tf * k1p1 / (tf + nd[d]) + delta);
        }
        __syncthreads();
      }
      // 4. select: documents 8 * tid .. 8 * tid + 7, byte tid & 3 of a word
      const f32x4 a0 = mine[0], a1 = mine[1];
      unsigned bits = 0xffu;
      if (allow != nullptr) {
        const long wi = tile * (BM_TILE / 32) + (tid >> 2);
        const unsigned word =
            wi < W ? allow[(long)(MQ > 1 ? q : 0) * W + wi] : 0u;
        bits = (word >> ((tid & 3) * 8)) & 0xffu;
      }
      // (scalars, not an array: an indexed array would live in scratch)
      unsigned pend = 0u;
#define BM_EACH(F) F(a0.x, 0) F(a0.y, 1) F(a0.z, 2) F(a0.w, 3) \
                   F(a1.x, 4) F(a1.y, 5) F(a1.z, 6) F(a1.w, 7)
#define BM_MARK(S, J) pend |= (S > 0.f && ((bits >> J) & 1u)) ? 1u << J : 0u;
      BM_EACH(BM_MARK)
      float* cs = cand_s + q * IDX_CAP;
      int* cr = cand_r + q * IDX_CAP;
      for (;;) {
        const float th = thr[q];
        bool crossed = false;
        auto offer = [&](float sj, int j) __attribute__((always_inline)) {
          if (!((pend >> j) & 1u)) return;
          if (sj >= th) {
            const int pos = atomicAdd(&cnt[q], 1);
            crossed |= pos >= lim;
            if (pos >= IDX_CAP) return;          // full: stays pending
            cs[pos] = sj;
            cr[pos] = (int)(d0 + 8 * tid + j);
          }
          pend &= ~(1u << j);
        };
#define BM_OFFER(S, J) offer(S, J);
        BM_EACH(BM_OFFER)
#undef BM_OFFER
#undef BM_MARK
#undef BM_EACH
        if (!__syncthreads_or((pend != 0u || crossed) ? 1 : 0)) break;
        if (w == 0) idx_compact(cs, cr, cnt + q, thr + q, k, lane);
        __syncthreads();
      }
    }
    __syncthreads();                             // nd, sl, qlive are reused
  }

  for (int qi = w; qi < Bg; qi += IDX_WAVES) {
    float* cs = cand_s + qi * IDX_CAP;
    int* cr = cand_r + qi * IDX_CAP;
    const int n = idx_compact(cs, cr, cnt + qi, thr + qi, k, lane);
    const long base = ((long)qi * gridDim.x + blockIdx.x) * k;
    for (int i = lane; i < k; i += WAVE) {
      ws_s[base + i] = i < n ? cs[i] : -INFINITY;
      ws_r[base + i] = i < n ? cr[i] : -1;
    }
  }
}

// ------------------------- MMR: fused Gram matrix and greedy selection
// mmr_select_kernel diversifies the candidate list of one query per block
// (8 waves): cand int64 [B, C], C <= 128, the rows a top-k kernel returned,
// -1 padding at the tail (a row outside [0, N) counts as padding).  All
// similarities come from the stored rows, fp16 or e4m3fn codes with a scale
// per row: rel_i = x_i . q and S_ij = x_i . x_j, fp32 sums of fp16 products
// (codes are multiplied unscaled, the scales multiply the finished sums).
//
// Gram phase.  D is walked in slabs of 128 dims.  Wave w gathers the slab of
// candidates 16w .. 16w+15: lane (c = l & 15, g = l >> 4) loads 16 bytes of
// row c per unit, four lanes covering 64 contiguous bytes, zeros for a
// padding row and past D.  For fp16 the four loads of a lane are its four A
// operands of mfma_f32_16x16x32_f16 (k = s*32 + g*8) as they stand; for
// e4m3fn two loads become four operands through idx_cvt8, which permutes k
// inside the slab.  The contraction order is free as long as every row and
// the query use the same one, and they do: a lane writes its operands to an
// LDS image [129 rows][128 halves, stride 272 B] at (row, s*64 + g*16), the
// query slab goes to row 128 through the same permutation, and every B
// operand is one conflict-free 16-byte read of that image.  The image is
// double-buffered: one block barrier per slab, the next slab's global loads
// issued before the barrier and in flight over the MFMAs.  Wave w owns row
// tile w against every column tile and the query (column 0 of a ninth
// tile): at most nine accumulators.  Tiles past the last valid candidate
// are skipped, loads and MFMAs alike.  The whole matrix is computed, not
// its upper triangle: that keeps the eight waves in step between barriers
// and leaves S complete, so the greedy phase reads rows only.
//
// Greedy phase.  The accumulators go to LDS over the dead images, S fp32
// [128][132] and rel [128], and wave 0 alone runs the k picks: lane l owns
// candidates l and l + 64 (rel, red and an open flag in registers), a pick
// is a wave arg-max over (objective desc, position asc), the update reads
// row p of S (contiguous: no bank conflict; S is symmetric) and the picks
// stay in registers, pick t in lane t & 63, until one coalesced store
// after the loop.  No atomics anywhere: the same inputs give the same bits.
#define MMR_CMAX 128
#define MMR_SLAB 128                           // dims of a slab
#define MMR_ROWB (MMR_SLAB * 2 + 16)           // image row stride, bytes
#define MMR_IMG ((MMR_CMAX + 1) * MMR_ROWB)    // candidates + the query
#define MMR_SLD (MMR_CMAX + 4)                 // S row stride, floats
#define MMR_LDS (2 * MMR_IMG + 3 * MMR_CMAX * 4 + 16)
static_assert(MMR_CMAX * MMR_SLD * 4 <= 2 * MMR_IMG, "S overlays the images");
static_assert(MMR_CMAX == IDX_WAVES * 16 && MMR_CMAX == 2 * WAVE,
              "a row tile per wave, two candidates per lane");

template <bool F16>
__launch_bounds__(IDX_WAVES * WAVE)
IDX_NO_PK_F32 __global__ void mmr_select_kernel(
    const char* __restrict__ rows, const float* __restrict__ scales,
    const _Float16* __restrict__ q, const long* __restrict__ cand,
    float* __restrict__ out_s, long* __restrict__ out_r, long N, int D, int C,
    int k, float lam, float oml) {
  constexpr int R = F16 ? 4 : 2;               // 16-byte loads per slab
  constexpr int EB = F16 ? 2 : 1;              // bytes per element
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* S = reinterpret_cast<float*>(smem);   // over the images, later
  float* rel = reinterpret_cast<float*>(smem + 2 * MMR_IMG);   // [128]
  float* sscale = rel + MMR_CMAX;                               // [128]
  int* crow = reinterpret_cast<int*>(sscale + MMR_CMAX);       // [128]
  unsigned long long* vmask =
      reinterpret_cast<unsigned long long*>(crow + MMR_CMAX);  // [2]

  const int tid = threadIdx.x;
  const int lane = tid & (WAVE - 1);
  const int w = tid / WAVE;
  const int c = lane & 15, g = lane >> 4;
  const long b = blockIdx.x;

  if (tid < MMR_CMAX) {
    long r = -1;
    if (tid < C) r = cand[b * C + tid];
    const bool ok = r >= 0 && r < N;
    crow[tid] = ok ? (int)r : -1;
    float sc = 1.f;
    if constexpr (!F16) sc = ok ? scales[r] : 0.f;
    sscale[tid] = sc;
    const unsigned long long bal = __ballot(ok);
    if (lane == 0) vmask[w] = bal;
  }
  __syncthreads();
  const unsigned long long v0 = vmask[0], v1 = vmask[1];
  // candidates up to the last valid one, in 16-row tiles
  const int nv = v1 ? 128 - __clzll((long long)v1)
                    : (v0 ? 64 - __clzll((long long)v0) : 0);
  const int NT = (nv + 15) >> 4;
  const bool live = w < NT;                    // wave-uniform
  const int myrow = crow[16 * w + c];
  const char* rp = rows + (long)(myrow < 0 ? 0 : myrow) * D * EB;
  const _Float16* qp = q + b * D;
  const int NSL = (D + MMR_SLAB - 1) / MMR_SLAB;

  // this lane's 16-byte units of a slab, and (first 16 threads) the query's;
  // the query unit of thread s*4 + g lands where operand s of lane group g
  // does, so it reads the k that the rows' permutation puts there
  // (the lambda must inline: a call would put the captures in scratch)
  auto load = [&](int slab, u32x4_t (&raw)[R], u32x4_t& qraw)
                  __attribute__((always_inline)) {
#pragma unroll
    for (int j = 0; j < R; ++j) {
      raw[j] = u32x4_t{0u, 0u, 0u, 0u};
      const int k0 = slab * MMR_SLAB + (F16 ? j * 32 + g * 8 : j * 64 + g * 16);
      if (live && myrow >= 0 && k0 < D)
        raw[j] = *reinterpret_cast<const u32x4_t*>(rp + (long)k0 * EB);
    }
    qraw = u32x4_t{0u, 0u, 0u, 0u};
    if (tid < 16) {
      const int s = tid >> 2, gq = tid & 3;
      const int kq = slab * MMR_SLAB +
                     (F16 ? s * 32 + gq * 8
                          : (s >> 1) * 64 + gq * 16 + (s & 1) * 8);
      if (kq < D) qraw = *reinterpret_cast<const u32x4_t*>(qp + kq);
    }
  };

  f32x4 acc[IDX_WAVES + 1];
#pragma unroll
  for (int t = 0; t <= IDX_WAVES; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  u32x4_t raw[R], qraw;
  load(0, raw, qraw);
  for (int slab = 0; slab < NSL; ++slab) {
    char* im = smem + (slab & 1) * MMR_IMG;
    f16x8_t a[4];
#pragma unroll
    for (int j = 0; j < R; ++j) {
      if constexpr (F16) {
        a[j] = __builtin_bit_cast(f16x8_t, raw[j]);
      } else {
        a[2 * j] = idx_cvt8(raw[j].x, raw[j].y);
        a[2 * j + 1] = idx_cvt8(raw[j].z, raw[j].w);
      }
    }
    if (live) {
#pragma unroll
      for (int s = 0; s < 4; ++s)
        *reinterpret_cast<f16x8_t*>(im + (16 * w + c) * MMR_ROWB + s * 64 +
                                    g * 16) = a[s];
    }
    if (tid < 16)
      *reinterpret_cast<u32x4_t*>(im + MMR_CMAX * MMR_ROWB + tid * 16) = qraw;
    if (slab + 1 < NSL) load(slab + 1, raw, qraw);
    __syncthreads();
    if (live) {
      // operands that hold data: fp16 k runs on, a 64-code unit of e4m3fn
      // spreads over two operands
      const int left = D - slab * MMR_SLAB;
      const int nst = min(4, F16 ? left / 32 : 2 * ((left + 63) / 64));
      const char* bp = im + c * MMR_ROWB + g * 16;
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        if (s < nst) {
#pragma unroll
          for (int t = 0; t < IDX_WAVES; ++t) {
            if (t < NT) {
              const f16x8_t bf = *reinterpret_cast<const f16x8_t*>(
                  bp + t * 16 * MMR_ROWB + s * 64);
              acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[s], bf, acc[t],
                                                              0, 0, 0);
            }
          }
          u32x4_t qb = {0u, 0u, 0u, 0u};
          if (c == 0)
            qb = *reinterpret_cast<const u32x4_t*>(
                im + MMR_CMAX * MMR_ROWB + s * 64 + g * 16);
          acc[IDX_WAVES] = __builtin_amdgcn_mfma_f32_16x16x32_f16(
              a[s], __builtin_bit_cast(f16x8_t, qb), acc[IDX_WAVES], 0, 0, 0);
        }
      }
    }
  }

  // lane (c, g) holds S[16w + 4g + r][16t + c] and, for c == 0, rel
  __syncthreads();                             // the images are dead
  if (live) {
    float si[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) si[r] = sscale[16 * w + 4 * g + r];
#pragma unroll
    for (int t = 0; t < IDX_WAVES; ++t) {
      if (t < NT) {
        const float sj = sscale[16 * t + c];
#pragma unroll
        for (int r = 0; r < 4; ++r)
          S[(16 * w + 4 * g + r) * MMR_SLD + 16 * t + c] =
              F16 ? acc[t][r] : acc[t][r] * (si[r] * sj);
      }
    }
    if (c == 0) {
#pragma unroll
      for (int r = 0; r < 4; ++r)
        rel[16 * w + 4 * g + r] =
            F16 ? acc[IDX_WAVES][r] : acc[IDX_WAVES][r] * si[r];
    }
  }
  __syncthreads();
  if (w != 0) return;

  // greedy picks: no block barrier and no global traffic inside the loop
  bool open0 = (v0 >> lane) & 1ull, open1 = (v1 >> lane) & 1ull;
  const float rel0 = open0 ? rel[lane] : 0.f;
  const float rel1 = open1 ? rel[lane + WAVE] : 0.f;
  float red0 = 0.f, red1 = 0.f;
  float ps0 = -INFINITY, ps1 = -INFINITY;      // picks lane and lane + 64
  int pp0 = -1, pp1 = -1;
  for (int t = 0; t < k; ++t) {
    // a closed candidate is (-inf, 255); an open one is never below the
    // largest negative float (NaN included), so it wins over a closed one
    float o0 = lam * rel0 - oml * red0, o1 = lam * rel1 - oml * red1;
    if (!(o0 >= -__FLT_MAX__)) o0 = -__FLT_MAX__;
    if (!(o1 >= -__FLT_MAX__)) o1 = -__FLT_MAX__;
    float best = open0 ? o0 : -INFINITY;
    int pos = open0 ? lane : 255;
    if (open1 && (!open0 || o1 > o0)) {
      best = o1;
      pos = lane + WAVE;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const float ob = __shfl_xor(best, off, WAVE);
      const int op = __shfl_xor(pos, off, WAVE);
      if (ob > best || (ob == best && op < pos)) {
        best = ob;
        pos = op;
      }
    }
    const int p = __builtin_amdgcn_readfirstlane(pos);
    if (p >= MMR_CMAX) break;                  // none left: the rest is padding
    if (lane == (t & (WAVE - 1))) {
      if (t < WAVE) {
        ps0 = rel[p];
        pp0 = crow[p];
      } else {
        ps1 = rel[p];
        pp1 = crow[p];
      }
    }
    if (p == lane) open0 = false;
    if (p == lane + WAVE) open1 = false;
    red0 = fmaxf(red0, S[p * MMR_SLD + lane]);
    red1 = fmaxf(red1, S[p * MMR_SLD + lane + WAVE]);
  }
  if (lane < k) {
    out_s[b * k + lane] = ps0;
    out_r[b * k + lane] = pp0;
  }
  if (lane + WAVE < k) {
    out_s[b * k + lane + WAVE] = ps1;
    out_r[b * k + lane + WAVE] = pp1;
  }
}

extern "C" {

hipError_t sentio_mmr_select(const void* q, const void* rows,
                             const float* scales, const long* cand,
                             float* out_s, long* out_r, long N, int D, int B,
                             int C, int k, float lam, hipStream_t stream) {
  if (N < 1 || N > 0x7fffffffL || D < 32 || D > 1024 || D % 32 || B < 1 ||
      C < 1 || C > MMR_CMAX || k < 1 || k > C || !(lam >= 0.f && lam <= 1.f) ||
      reinterpret_cast<uintptr_t>(q) % 16 ||
      reinterpret_cast<uintptr_t>(rows) % 16)
    return hipErrorInvalidValue;
  static_assert(SENTIO_MMR_MAX_C == MMR_CMAX, "limit of the header");
  auto kern = scales == nullptr ? mmr_select_kernel<true>
                                : mmr_select_kernel<false>;
  hipError_t e = hipFuncSetAttribute(
      reinterpret_cast<const void*>(kern),
      hipFuncAttributeMaxDynamicSharedMemorySize, MMR_LDS);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(kern, dim3((unsigned)B), dim3(IDX_WAVES * WAVE), MMR_LDS,
                     stream, (const char*)rows, scales, (const _Float16*)q,
                     cand, out_s, out_r, N, D, C, k, lam, 1.f - lam);
  HIP_CHECK_LAUNCH();
  return hipSuccess;
}

hipError_t sentio_bm25_topk_plan(long N, int* blocks, int* tile_docs,
                                 int* cap) {
  int dev = 0, cus = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
  if (e != hipSuccess) return e;
  if (N < 1 || cus < 1) return hipErrorInvalidValue;
  const long tiles = (N + BM_TILE - 1) / BM_TILE;
  long nb = cus < IDX_MAX_BLOCKS ? cus : IDX_MAX_BLOCKS;
  if (nb > tiles) nb = tiles;
  *blocks = (int)nb;
  *tile_docs = BM_TILE;
  *cap = IDX_CAP;
  return hipSuccess;
}

hipError_t sentio_bm25_topk(const long* tids, const int* qoff,
                            const long* indptr, const int* post_doc,
                            const float* post_tf, const float* idf,
                            const float* doc_len, const int* allow,
                            int mask_rows, float* ws_s, int* ws_r,
                            float* out_s, long* out_r, long N, long n_terms,
                            int B, int TT, int k, int blocks, float k1,
                            float b, float avgdl, float delta,
                            hipStream_t stream) {
  if (N < 1 || N > 0x7fffffffL || B < 1 || B > SENTIO_BM25_TOPK_MAX_B ||
      TT < 0 || TT > SENTIO_BM25_TOPK_MAX_TERMS || k < 1 || k > IDX_KMAX ||
      blocks < 1 || blocks > IDX_MAX_BLOCKS ||
      blocks > (N + BM_TILE - 1) / BM_TILE || n_terms < 0 || !(avgdl > 0.f) ||
      (allow != nullptr && ((mask_rows != 1 && mask_rows != B) ||
                            reinterpret_cast<uintptr_t>(allow) % 16)))
    return hipErrorInvalidValue;
  static_assert(SENTIO_BM25_TOPK_MAX_TERMS == BM_MAX_TERMS &&
                SENTIO_BM25_TOPK_MAX_B == 32 &&
                SENTIO_BM25_TOPK_MAX_K == IDX_KMAX, "limits of the header");
  const size_t lds = (size_t)2 * BM_TILE * 4 + (size_t)BM_MAX_TERMS * (16 + 4) +
                     (size_t)B * IDX_CAP * 8 + (32 + 32 + 33 + 32 + 32) * 4;
  hipError_t e = hipFuncSetAttribute(
      reinterpret_cast<const void*>(bm25_topk_kernel),
      hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(bm25_topk_kernel, dim3((unsigned)blocks),
                     dim3(BM_THREADS), lds, stream, tids, qoff, indptr,
                     post_doc, post_tf, idf, doc_len, (const unsigned*)allow,
                     allow ? mask_rows : 1, ws_s, ws_r, N, n_terms, B, TT, k,
                     k1, b, 1.f / avgdl, delta);
  HIP_CHECK_LAUNCH();
  hipLaunchKernelGGL(index_merge_kernel, dim3((unsigned)B),
                     dim3(IDX_MERGE_THREADS), 0, stream, ws_s, ws_r, out_s,
                     out_r, blocks * k, k);
  HIP_CHECK_LAUNCH();
  return hipSuccess;
}

hipError_t sentio_cosine_topk_fp8_plan(long N, int* blocks, int* chunk_rows,
                                       int* cap) {
  int dev = 0, cus = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
  if (e != hipSuccess) return e;
  if (N < 1 || cus < 1) return hipErrorInvalidValue;
  const long chunks = (N + IDX_CHUNK - 1) / IDX_CHUNK;
  long b = cus < IDX_MAX_BLOCKS ? cus : IDX_MAX_BLOCKS;
  if (b > chunks) b = chunks;
  *blocks = (int)b;
  *chunk_rows = IDX_CHUNK;
  *cap = IDX_CAP;
  return hipSuccess;
}

hipError_t sentio_cosine_topk_fp8(const void* q, const void* codes,
                                  const float* scales, float* ws_s, int* ws_r,
                                  float* out_s, long* out_r, long N, int D,
                                  int B, int k, int blocks,
                                  hipStream_t stream) {
  if (N < 1 || N > 0x7fffffffL || D < 32 || D > 1024 || D % 32 || B < 1 ||
      k < 1 || k > IDX_KMAX || blocks < 1 || blocks > IDX_MAX_BLOCKS)
    return hipErrorInvalidValue;
  for (int b0 = 0; b0 < B; b0 += 32) {
    const int Bg = B - b0 < 32 ? B - b0 : 32;
    const void* qg = (const char*)q + (size_t)b0 * D * 2;
    hipError_t e;
    if (D == 1024)
      e = Bg > 16 ? launch_index_scan<2, 16>(qg, codes, scales, ws_s, ws_r, N,
                                             D, Bg, k, b0, blocks, stream)
                  : launch_index_scan<1, 16>(qg, codes, scales, ws_s, ws_r, N,
                                             D, Bg, k, b0, blocks, stream);
    else
      e = Bg > 16 ? launch_index_scan<2, 0>(qg, codes, scales, ws_s, ws_r, N,
                                            D, Bg, k, b0, blocks, stream)
                  : launch_index_scan<1, 0>(qg, codes, scales, ws_s, ws_r, N,
                                            D, Bg, k, b0, blocks, stream);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(index_merge_kernel, dim3((unsigned)B),
                     dim3(IDX_MERGE_THREADS), 0, stream, ws_s, ws_r, out_s,
                     out_r, blocks * k, k);
  HIP_CHECK_LAUNCH();
  return hipSuccess;
}

hipError_t sentio_cosine_topk_masked(const void* q, const void* rows,
                                     const float* scales, const int* allow,
                                     int mask_rows, float* ws_s, int* ws_r,
                                     float* out_s, long* out_r, long N, int D,
                                     int B, int k, int blocks,
                                     hipStream_t stream) {
  if (N < 1 || N > 0x7fffffffL || D < 32 || D > 1024 || D % 32 || B < 1 ||
      k < 1 || k > IDX_KMAX || blocks < 1 || blocks > IDX_MAX_BLOCKS ||
      (mask_rows != 1 && mask_rows != B) || allow == nullptr ||
      reinterpret_cast<uintptr_t>(allow) % 16)
    return hipErrorInvalidValue;
  const long W = 4 * ((N + IDX_CHUNK - 1) / IDX_CHUNK);
  for (int b0 = 0; b0 < B; b0 += 32) {
    const int Bg = B - b0 < 32 ? B - b0 : 32;
    const void* qg = (const char*)q + (size_t)b0 * D * 2;
    const int* ag = mask_rows == 1 ? allow : allow + (long)b0 * W;
    const int MQ = mask_rows == 1 ? 1 : Bg;
#define IDX_MASKED(ET, NU)                                                   \
  (Bg > 16 ? launch_index_scan_masked<ET, 2, NU>(qg, rows, scales, ag, MQ,   \
                                                 ws_s, ws_r, N, D, Bg, k,    \
                                                 b0, blocks, stream)         \
           : launch_index_scan_masked<ET, 1, NU>(qg, rows, scales, ag, MQ,   \
                                                 ws_s, ws_r, N, D, Bg, k,    \
                                                 b0, blocks, stream))
    hipError_t e;
    if (scales == nullptr)
      e = IDX_MASKED(_Float16, 0);
    else if (D == 1024)
      e = IDX_MASKED(unsigned char, 16);
    else
      e = IDX_MASKED(unsigned char, 0);
#undef IDX_MASKED
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(index_merge_kernel, dim3((unsigned)B),
                     dim3(IDX_MERGE_THREADS), 0, stream, ws_s, ws_r, out_s,
                     out_r, blocks * k, k);
  HIP_CHECK_LAUNCH();
  return hipSuccess;
}

hipError_t sentio_cosine_scores_f16(const void* mat, const void* q,
                                    float* scores, long N, int D, int B,
                                    hipStream_t stream) {
  return launch_cosine<_Float16>(mat, q, scores, N, D, B, stream);
}

hipError_t sentio_cosine_scores_bf16(const void* mat, const void* q,
                                     float* scores, long N, int D, int B,
                                     hipStream_t stream) {
  return launch_cosine<__bf16>(mat, q, scores, N, D, B, stream);
}

hipError_t sentio_bm25(const long* term_ids, const long* qoff,
                       const long* starts, const int* post_doc,
                       const float* post_tf, const float* idf,
                       const float* doc_len, float* scores, int T, long total,
                       float k1, float b, float avgdl, float delta,
                       hipStream_t stream) {
  if (total == 0) return hipSuccess;
  long blocks = (total + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(bm25_kernel, dim3((unsigned)blocks), dim3(256), 0, stream,
                     term_ids, qoff, starts, post_doc, post_tf, idf, doc_len,
                     scores, T, total, k1, b, 1.f / avgdl, delta);
  HIP_CHECK_LAUNCH();
  return hipSuccess;
}

hipError_t sentio_fuse_topk(const long* d_ids, const float* d_scores,
                            const long* s_ids, const float* s_scores,
                            long* out_ids, float* out_scores, int B, int Kd,
                            int Ks, int top_k, int method, float rrf_k,
                            float dw, float sw, hipStream_t stream) {
  if (Kd + Ks > FUSE_MAX || top_k > FUSE_MAX) return hipErrorInvalidValue;
  hipLaunchKernelGGL(fuse_topk_kernel, dim3(B), dim3(128), 0, stream, d_ids,
                     d_scores, s_ids, s_scores, out_ids, out_scores, Kd, Ks,
                     top_k, method, rrf_k, dw, sw);
  HIP_CHECK_LAUNCH();
  return hipSuccess;
}

}  // extern "C"
