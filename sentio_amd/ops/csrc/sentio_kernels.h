// C API of the sentio gfx950 kernels: every extern "C" entry point, declared
// once.  Each kernel TU includes this next to its definitions and
// bindings.hip includes it for its calls; extern "C" functions cannot be
// overloaded, so a definition or call that disagrees with a declaration
// here is a compile error instead of a silently mis-linked symbol.
// All pointers are device pointers; launches go to `stream`.
#pragma once

#include <hip/hip_runtime.h>

extern "C" {

// ---- elementwise.hip
hipError_t sentio_rmsnorm(const void* x, const void* w, void* y, long rows,
                          int D, float eps, hipStream_t stream);
hipError_t sentio_rmsnorm_residual(const void* x, const void* res,
                                   const void* w, void* y, void* h, long rows,
                                   int D, float eps, hipStream_t stream);
// part is fp32 [S, rows, D], slabs summed in increasing s; S sits BEFORE
// rows and D; writes y and h like sentio_rmsnorm_residual.  Rows of at most
// 8192 elements keep h in registers between the passes; reread != 0 takes
// the kernel that loads h back at any row length (tests and probes).
// Outputs are bit-identical
hipError_t sentio_rmsnorm_residual_partials(const float* part, const void* res,
                                            const void* w, void* y, void* h,
                                            int S, long rows, int D, float eps,
                                            int reread, hipStream_t stream);
hipError_t sentio_swiglu(const void* gate, const void* up, void* out, long n,
                         hipStream_t stream);
// F is the OUTPUT width (half the packed [gate | up] row)
hipError_t sentio_swiglu_packed(const void* gu, void* out, long rows, int F,
                                hipStream_t stream);
hipError_t sentio_rope(const void* x, void* y, const float* cosT,
                       const float* sinT, const int* pos, int B, int S, int H,
                       int D, hipStream_t stream);
// trailing dims are (D, Smax) here but (Smax, D) in the attention entry points
hipError_t sentio_decode_qkv_prep(const void* qkv, void* q_out, void* kc,
                                  void* vc, const float* cosT,
                                  const float* sinT, const int* seq_lens,
                                  int B, int H, int Hkv, int D, int Smax,
                                  hipStream_t stream);
// qkv is [B, S, (H+2*Hkv)*D]; token (b, s) sits at position pos0 + s.
// Smax > 0: k_out / v_out are caches [Bc, Hkv, Smax, D], rows pos0 ..
// pos0+S-1 of batch rows 0 .. B-1 are written; Smax == 0: contiguous
// [B, S, Hkv, D] outputs (Bc ignored).  hipErrorInvalidValue unless
// D % 8 == 0, pos0 >= 0, pos0 + S <= table_rows and, with caches,
// pos0 + S <= Smax and Bc >= B.  Every pointer must be 16-byte aligned
hipError_t sentio_prefill_qkv_prep(const void* qkv, void* q_out, void* k_out,
                                   void* v_out, const float* cosT,
                                   const float* sinT, int B, int S, int H,
                                   int Hkv, int D, int Bc, int Smax, int pos0,
                                   int table_rows, hipStream_t stream);
hipError_t sentio_softmax(const void* x, void* y, long rows, int D,
                          hipStream_t stream);
hipError_t sentio_mean_pool_l2norm(const void* hidden,
                                   const unsigned char* mask, float* out,
                                   int B, int S, int D, hipStream_t stream);
hipError_t sentio_sample(const float* logits, long* out, float* ws_val,
                         int* ws_idx, int B, int V, float temperature,
                         unsigned seed, hipStream_t stream);

// ---- sampling.hip
hipError_t sentio_sample_support(const float* logits, const float* temperature,
                                 const int* top_k, const float* top_p,
                                 float* tau, int* count, long B, int V,
                                 hipStream_t stream);
hipError_t sentio_sample_filtered(const float* logits, const float* temperature,
                                  const int* top_k, const float* top_p,
                                  const long* seed, const int* step, long* out,
                                  long B, int V, hipStream_t stream);
// logits [R,V]; slot [R] or null (null: R == S, row r is slot r); the
// parameter arrays, step (in/out) and tok (in/out) are [S]; active [S] or
// null; dims are (R, S, V).  Rows whose slot is outside [0,S) or inactive
// write nothing
hipError_t sentio_sample_slots(const float* logits, const int* slot,
                               const float* temperature, const int* top_k,
                               const float* top_p, const long* seed, int* step,
                               const unsigned char* active, long* tok, long R,
                               int S, int V, hipStream_t stream);
// grammar-constrained sample_filtered.  state / left are int32 [B], in/out;
// next int16 [N, Vt], mask int32 [N, W] with W == ceil(Vt/32), dist int16
// [N]; max_dist >= every dist entry.  A row with state in [0, N) draws only
// from v < min(V, Vt) with mask bit v set and dist[next[state, v]] <=
// left - 1, then state = next[state, tok], left -= 1; any other state is
// sampled unconstrained and keeps state and left.  Dims are (B, V, Vt, N,
// W, max_dist); hipErrorInvalidValue unless 1 <= N <= 32767, W matches Vt
// and W <= 2048
hipError_t sentio_sample_constrained(
    const float* logits, const float* temperature, const int* top_k,
    const float* top_p, const long* seed, const int* step, int* state,
    int* left, const short* next, const int* mask, const short* dist,
    long* tok, long B, int V, int Vt, int N, int W, int max_dist,
    hipStream_t stream);
// sentio_sample_slots with per-slot state / left [S]; the tables follow
// them, dims are (R, S, V, Vt, N, W, max_dist)
hipError_t sentio_sample_slots_constrained(
    const float* logits, const int* slot, const float* temperature,
    const int* top_k, const float* top_p, const long* seed, int* step,
    const unsigned char* active, long* tok, int* state, int* left,
    const short* next, const int* mask, const short* dist, long R, int S,
    int V, int Vt, int N, int W, int max_dist, hipStream_t stream);
// sample_filtered over logits [B, V] rewritten by repetition / frequency /
// presence penalties.  out_buf int64 [B, L] holds each row's emitted tokens,
// out_len int32 [B] of them valid (clamped to [0, L]; ids outside [0, V)
// are ignored); rep / freq / pres are f32 [B].  A token with count c > 0
// samples from x = (x < 0 ? x * rep : x / rep) - freq * c - pres, each
// operation rounded on its own.  In: logits, temperature, top_k, top_p,
// seed, rep, freq, pres.  In/out: step (+= 1), out_buf and out_len (the
// token is appended while 0 <= out_len[b] < L, else both are kept).  Out:
// tok int64 [B].  Dims are (B, V, L); hipErrorInvalidValue unless
// 1 <= B <= 2^31 - 1, 1 <= V < 2^18 and 1 <= L <= 4096
hipError_t sentio_sample_penalized(
    const float* logits, const float* temperature, const int* top_k,
    const float* top_p, const long* seed, int* step, long* out_buf,
    int* out_len, const float* rep, const float* freq, const float* pres,
    long* tok, long B, int V, int L, hipStream_t stream);
// prompt-lookup draft: hist int64 [B, L], hist_len / room int32 [B] ->
// draft int64 [B, K], n_draft int32 [B]; dims are (B, L, K, n_max)
hipError_t sentio_ngram_draft(const long* hist, const int* hist_len,
                              const int* room, long* draft, int* n_draft,
                              int B, int L, int K, int n_max,
                              hipStream_t stream);
// speculative accept, in place on out_buf [B, OW], out_len, hist [B, L],
// hist_len, seq_lens, cur and stats int32 [B, 2]; sampled int64 [B, T],
// draft int64 [B, T-1]; room int32 [B] or null; dims are (B, T, OW, L,
// max_new, smax)
hipError_t sentio_spec_accept(const long* sampled, const long* draft,
                              const int* n_draft, long* out_buf, int* out_len,
                              long* hist, int* hist_len, int* seq_lens,
                              long* cur, int* stats, int* room, int B, int T,
                              int OW, int L, int max_new, int smax,
                              hipStream_t stream);

// ---- retrieval.hip
// index matrix first, queries second; dims are (N, D, B)
hipError_t sentio_cosine_scores_f16(const void* mat, const void* q,
                                    float* scores, long N, int D, int B,
                                    hipStream_t stream);
hipError_t sentio_cosine_scores_bf16(const void* mat, const void* q,
                                     float* scores, long N, int D, int B,
                                     hipStream_t stream);
// launch plan of sentio_cosine_topk_fp8 on the current device for N rows:
// scan blocks (one per CU, at most 256, at most one per chunk), rows per
// block chunk, places per query in a block's candidate list
hipError_t sentio_cosine_topk_fp8_plan(long N, int* blocks, int* chunk_rows,
                                       int* cap);
// queries first here: q fp16 [B, D], codes uint8 (e4m3fn) [N, D], scales
// fp32 [N]; ws_s / ws_r hold B * blocks * k places; out_s f32 / out_r i64
// [B, k], sorted by (score desc, row asc), (-inf, -1) past N; dims are (N,
// D, B, k, blocks).  hipErrorInvalidValue unless D % 32 == 0, 32 <= D <=
// 1024, 1 <= k <= 128, N < 2^31 and 1 <= blocks <= 256.  q and codes must
// be 16-byte aligned
hipError_t sentio_cosine_topk_fp8(const void* q, const void* codes,
                                  const float* scales, float* ws_s, int* ws_r,
                                  float* out_s, long* out_r, long N, int D,
                                  int B, int k, int blocks,
                                  hipStream_t stream);
// the same search over the rows that a bit mask allows.  rows: e4m3fn codes
// [N, D] with scales fp32 [N], or fp16 [N, D] when scales is null.  allow
// int32 [mask_rows, W], mask_rows 1 (one mask for every query) or B, W = 4 *
// ceil(N / 128); row n is bit n & 31 of word n >> 5; bits at or past N are
// ignored.  Out as above, (-inf, -1) past the number of allowed rows.  The
// plan, the workspace and the conditions are those of sentio_cosine_topk_fp8;
// also hipErrorInvalidValue unless mask_rows is 1 or B and allow is 16-byte
// aligned
hipError_t sentio_cosine_topk_masked(const void* q, const void* rows,
                                     const float* scales, const int* allow,
                                     int mask_rows, float* ws_s, int* ws_r,
                                     float* out_s, long* out_r, long N, int D,
                                     int B, int k, int blocks,
                                     hipStream_t stream);
// MMR over a candidate list, one block per query: q fp16 [B, D]; rows as in
// sentio_cosine_topk_masked (e4m3fn codes with scales, or fp16 when scales
// is null); cand int64 [B, C], index rows, unique within a list, -1 padding
// at the tail (a row outside [0, N) counts as padding).  Step t picks the
// unpicked valid candidate with the largest lam * (x_i . q) - (1 - lam) *
// max over the picks p of (x_i . x_p), a tie to the lower position in cand;
// all dot products are fp32 sums over the stored values.  out_s f32 [B, k]:
// x_p . q of each pick, out_r i64 [B, k]: its index row, in pick order,
// (-inf, -1) past the valid candidates; deterministic.  dims are (N, D, B,
// C, k).  hipErrorInvalidValue unless D % 32 == 0, 32 <= D <= 1024, 1 <= C
// <= 128, 1 <= k <= C, 0 <= lam <= 1, N < 2^31 and q and rows are 16-byte
// aligned
#define SENTIO_MMR_MAX_C 128
hipError_t sentio_mmr_select(const void* q, const void* rows,
                             const float* scales, const long* cand,
                             float* out_s, long* out_r, long N, int D, int B,
                             int C, int k, float lam, hipStream_t stream);
hipError_t sentio_bm25(const long* term_ids, const long* qoff,
                       const long* starts, const int* post_doc,
                       const float* post_tf, const float* idf,
                       const float* doc_len, float* scores, int T, long total,
                       float k1, float b, float avgdl, float delta,
                       hipStream_t stream);
// limits of one sentio_bm25_topk launch
#define SENTIO_BM25_TOPK_MAX_B 32        // queries
#define SENTIO_BM25_TOPK_MAX_K 128       // results per query
#define SENTIO_BM25_TOPK_MAX_TERMS 1024  // query terms, summed over queries
// launch plan of sentio_bm25_topk on the current device for N documents:
// blocks (one per CU, at most 256, at most one per tile), documents per
// tile, places per query in a block's candidate list
hipError_t sentio_bm25_topk_plan(long N, int* blocks, int* tile_docs,
                                 int* cap);
// batched BM25 search with the top-k fused into the scoring: no score array
// in global memory.  Query b has the term ids tids[qoff[b] .. qoff[b+1])
// (int64 [TT], qoff int32 [B+1], qoff[0] == 0, qoff[B] == TT; a term given
// twice counts twice; an id outside [0, n_terms) has no postings).  CSR
// index: indptr int64 [n_terms+1], post_doc int32, post_tf fp32, idf fp32
// [n_terms], doc_len fp32 [N].  INVARIANT: within [indptr[t], indptr[t+1])
// post_doc is strictly ascending (sorted by document, a document at most
// once per term); the kernel finds a tile's postings by binary search and
// adds them without atomics.  score = sum over the query's terms, in query
// order, of idf * (tf * (k1 + 1) / (tf + k1 * (1 - b + b * doc_len /
// avgdl)) + delta).  allow: null, or the row mask of
// sentio_cosine_topk_masked (int32 [mask_rows, W], mask_rows 1 or B, W = 4 *
// ceil(N / 128), bits at or past N ignored, 16-byte aligned).  out_s f32 /
// out_r i64 [B, k]: the allowed documents with score > 0, sorted by (score
// desc, row asc), (-inf, -1) past their number; deterministic.  ws_s / ws_r
// hold B * blocks * k places.  hipErrorInvalidValue unless 1 <= B <= 32, 0
// <= TT <= 1024, 1 <= k <= 128, 1 <= N < 2^31, avgdl > 0 and 1 <= blocks <=
// min(256, tiles)
hipError_t sentio_bm25_topk(const long* tids, const int* qoff,
                            const long* indptr, const int* post_doc,
                            const float* post_tf, const float* idf,
                            const float* doc_len, const int* allow,
                            int mask_rows, float* ws_s, int* ws_r,
                            float* out_s, long* out_r, long N, long n_terms,
                            int B, int TT, int k, int blocks, float k1,
                            float b, float avgdl, float delta,
                            hipStream_t stream);
hipError_t sentio_fuse_topk(const long* d_ids, const float* d_scores,
                            const long* s_ids, const float* s_scores,
                            long* out_ids, float* out_scores, int B, int Kd,
                            int Ks, int top_k, int method, float rrf_k,
                            float dw, float sw, hipStream_t stream);

// ---- attention.hip
hipError_t sentio_flash_attn(const void* q, const void* k, const void* v,
                             void* out, const int* kv_lens, int B, int S,
                             int H, int Hkv, int D, float scale, int causal,
                             hipStream_t stream);
// Smax sits BEFORE D here; always causal, q_off replaces the causal flag
hipError_t sentio_flash_attn_cache(const void* q, const void* kc,
                                   const void* vc, void* out,
                                   const int* kv_lens, int B, int S, int H,
                                   int Hkv, int Smax, int D, float scale,
                                   int q_off, hipStream_t stream);
// splits and waves (block width, 4 or 8) come BEFORE the shape; no S (one
// query token per row); ws_o/ws_ml may be null when splits == 1
hipError_t sentio_decode_attn(const void* q, const void* kc, const void* vc,
                              void* out, const int* seq_lens, float* ws_o,
                              float* ws_ml, int splits, int waves, int B,
                              int H, int Hkv, int Smax, int D, float scale,
                              hipStream_t stream);
// as sentio_decode_attn, but the first argument is the raw QKV projection
// [B, (H+2*Hkv)*D], the caches are WRITTEN (row seq_lens[b]), and the RoPE
// tables sit between out and seq_lens; seq_lens is the new token's position
hipError_t sentio_decode_attn_fused(const void* qkv, void* kc, void* vc,
                                    void* out, const float* cosT,
                                    const float* sinT, const int* seq_lens,
                                    float* ws_o, float* ws_ml, int splits,
                                    int waves, int B, int H, int Hkv,
                                    int Smax, int D, float scale,
                                    hipStream_t stream);
// as sentio_decode_attn_fused over uint8 (e4m3fn) caches; the four fp32
// [Hkv] scale arrays sit between seq_lens and the workspaces, in the order
// k_scale, v_scale, then the reciprocals k_inv, v_inv
hipError_t sentio_decode_attn_fused_fp8(
    const void* qkv, void* kc, void* vc, void* out, const float* cosT,
    const float* sinT, const int* seq_lens, const float* k_scale,
    const float* v_scale, const float* k_inv, const float* v_inv, float* ws_o,
    float* ws_ml, int splits, int waves, int B, int H, int Hkv, int Smax,
    int D, float scale, hipStream_t stream);
// as sentio_decode_attn_fused for T tokens per batch row (2 <= T <= 8,
// (H/Hkv)*T <= 32): qkv is [B*T, (H+2*Hkv)*D], row b*T + t sits at position
// seq_lens[b] + t; out is [B*T, H*D]; T sits between B and H.  With
// splits > 1 the workspaces hold B*T "batch rows" of partials
hipError_t sentio_decode_attn_verify(const void* qkv, void* kc, void* vc,
                                     void* out, const float* cosT,
                                     const float* sinT, const int* seq_lens,
                                     float* ws_o, float* ws_ml, int splits,
                                     int waves, int B, int T, int H, int Hkv,
                                     int Smax, int D, float scale,
                                     hipStream_t stream);
// bf16 sources [n, Hkv, S_src, D] -> uint8 caches [B, Hkv, Smax, D] at
// rows[i], first S rows; reciprocals only; dims are (n, B, Hkv, S_src, S,
// Smax, D) — S_src and S sit BEFORE Smax
hipError_t sentio_kv_store_fp8(const void* src_k, const void* src_v,
                               void* dst_k, void* dst_v, const int* rows,
                               const float* k_inv, const float* v_inv, int n,
                               int B, int Hkv, int S_src, int S, int Smax,
                               int D, hipStream_t stream);

// ---- gemm.hip / blaslt.hip
// B is [K, N] row-major; dims are (M, N, K)
hipError_t sentio_gemm_bf16(const void* A, const void* B, void* C, int M,
                            int N, int K, hipStream_t stream);
// w is [N, K] row-major (TN); dims are (M, K, N) — NOT (M, N, K)
hipError_t sentio_skinny_gemm(const void* x, const void* w, void* out, int M,
                              int K, int N, hipStream_t stream);
// split-K partials: w is [N, K] row-major (TN), part is fp32 [S, M, N];
// dims are (M, K, N, S) like skinny_gemm.  hipErrorInvalidValue unless
// 1 <= M <= 32, N % 64 == 0 and K % (32 * S) == 0
hipError_t sentio_decode_gemm_splitk(const void* x, const void* w, float* part,
                                     int M, int K, int N, int S,
                                     hipStream_t stream);
// w is [N, K] row-major (TN) like skinny_gemm, but dims are (M, N, K);
// returns 0 on success, not a hipError_t
int sentio_lt_gemm_tn(const void* x, const void* w, void* out, int M, int N,
                      int K, hipStream_t stream);

}  // extern "C"
