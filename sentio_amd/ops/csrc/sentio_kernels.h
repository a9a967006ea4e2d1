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

// ---- retrieval.hip
// index matrix first, queries second; dims are (N, D, B)
hipError_t sentio_cosine_scores_f16(const void* mat, const void* q,
                                    float* scores, long N, int D, int B,
                                    hipStream_t stream);
hipError_t sentio_cosine_scores_bf16(const void* mat, const void* q,
                                     float* scores, long N, int D, int B,
                                     hipStream_t stream);
hipError_t sentio_bm25(const long* term_ids, const long* qoff,
                       const long* starts, const int* post_doc,
                       const float* post_tf, const float* idf,
                       const float* doc_len, float* scores, int T, long total,
                       float k1, float b, float avgdl, float delta,
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
