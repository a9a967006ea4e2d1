// Torch bindings for the sentio gfx950 kernels.  The only TU that includes
// torch headers (slow compile); the kernels live in the sibling .hip TUs and
// are called through the C API declared in sentio_kernels.h, which those
// TUs include too, so the compiler checks every call here against the
// definitions.
#include <torch/extension.h>
#include <c10/hip/HIPStream.h>
#include <hip/hip_runtime.h>
#include <cstdlib>
#include <limits>
#include <tuple>

#include "sentio_kernels.h"

namespace {

void check_hip(hipError_t e, const char* what) {
  TORCH_CHECK(e == hipSuccess, "sentio HIP kernel '", what,
              "' failed: ", hipGetErrorString(e));
}

hipStream_t stream() {
  return c10::hip::getCurrentHIPStream().stream();
}

void check_bf16_cuda(const torch::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda(), name, " must be on GPU");
  TORCH_CHECK(t.scalar_type() == torch::kBFloat16, name, " must be bf16");
  TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
}

torch::Tensor rmsnorm(torch::Tensor x, torch::Tensor w, double eps) {
  check_bf16_cuda(x, "x");
  check_bf16_cuda(w, "w");
  const int D = x.size(-1);
  const long rows = x.numel() / D;
  auto y = torch::empty_like(x);
  check_hip(sentio_rmsnorm(x.data_ptr(), w.data_ptr(), y.data_ptr(), rows, D,
                           (float)eps, stream()), "rmsnorm");
  return y;
}

std::vector<torch::Tensor> rmsnorm_residual(torch::Tensor x, torch::Tensor res,
                                            torch::Tensor w, double eps) {
  check_bf16_cuda(x, "x");
  const int D = x.size(-1);
  const long rows = x.numel() / D;
  auto y = torch::empty_like(x);
  auto h = torch::empty_like(x);
  check_hip(sentio_rmsnorm_residual(x.data_ptr(), res.data_ptr(), w.data_ptr(),
                                    y.data_ptr(), h.data_ptr(), rows, D,
                                    (float)eps, stream()), "rmsnorm_residual");
  return {y, h};
}

torch::Tensor swiglu(torch::Tensor gate, torch::Tensor up) {
  check_bf16_cuda(gate, "gate");
  auto out = torch::empty_like(gate);
  check_hip(sentio_swiglu(gate.data_ptr(), up.data_ptr(), out.data_ptr(),
                          gate.numel(), stream()), "swiglu");
  return out;
}

torch::Tensor swiglu_packed(torch::Tensor gu) {
  check_bf16_cuda(gu, "gu");
  const int F2 = gu.size(-1);
  TORCH_CHECK(F2 % 16 == 0, "packed width must be divisible by 16");
  const long rows = gu.numel() / F2;
  auto sizes = gu.sizes().vec();
  sizes.back() = F2 / 2;
  auto out = torch::empty(sizes, gu.options());
  check_hip(sentio_swiglu_packed(gu.data_ptr(), out.data_ptr(), rows, F2 / 2,
                                 stream()), "swiglu_packed");
  return out;
}

torch::Tensor rope_apply(torch::Tensor x, torch::Tensor cosT, torch::Tensor sinT,
                         torch::Tensor pos) {
  check_bf16_cuda(x, "x");
  TORCH_CHECK(x.dim() == 4, "x must be [B,S,H,D]");
  TORCH_CHECK(cosT.scalar_type() == torch::kFloat, "cos table must be f32");
  auto pos_i = pos.to(torch::kInt).contiguous();
  auto y = torch::empty_like(x);
  check_hip(sentio_rope(x.data_ptr(), y.data_ptr(),
                        cosT.data_ptr<float>(), sinT.data_ptr<float>(),
                        pos_i.data_ptr<int>(), x.size(0), x.size(1), x.size(2),
                        x.size(3), stream()), "rope");
  return y;
}

torch::Tensor decode_qkv_prep(torch::Tensor qkv, torch::Tensor kc,
                              torch::Tensor vc, torch::Tensor cosT,
                              torch::Tensor sinT, torch::Tensor seq_lens) {
  check_bf16_cuda(qkv, "qkv");
  TORCH_CHECK(qkv.dim() == 2, "qkv must be [B, (H+2*Hkv)*D]");
  TORCH_CHECK(kc.dim() == 4 && vc.dim() == 4, "caches must be [B,Hkv,Smax,D]");
  TORCH_CHECK(seq_lens.scalar_type() == torch::kInt, "seq_lens must be i32");
  const int B = qkv.size(0);
  const int Hkv = kc.size(1);
  const int Smax = kc.size(2);
  const int D = kc.size(3);
  const int H = (int)(qkv.size(1) / D) - 2 * Hkv;
  TORCH_CHECK(H > 0 && (long)(H + 2 * Hkv) * D == qkv.size(1),
              "qkv width mismatch");
  auto q_out = torch::empty({B, H, D}, qkv.options());
  check_hip(sentio_decode_qkv_prep(qkv.data_ptr(), q_out.data_ptr(),
                                   kc.data_ptr(), vc.data_ptr(),
                                   cosT.data_ptr<float>(),
                                   sinT.data_ptr<float>(),
                                   seq_lens.data_ptr<int>(), B, H, Hkv, D,
                                   Smax, stream()), "decode_qkv_prep");
  return q_out;
}

void check_caches(const torch::Tensor& kc, const torch::Tensor& vc);

// Prefill head prep in one launch: split the raw QKV projection
// [B, S, (H+2*Hkv)*D], RoPE q and k at positions pos0 + s, and write k / v
// into the caches' rows pos0 .. pos0+S-1 (returns {q}) or, without caches,
// into new contiguous tensors (returns {q, k, v}).  Everything is checked
// before the launch; nothing synchronises, so it can be graph-captured.
std::vector<torch::Tensor> prefill_qkv_prep(
    torch::Tensor qkv, torch::Tensor cosT, torch::Tensor sinT, int64_t pos0,
    int64_t H, int64_t Hkv, c10::optional<torch::Tensor> kc,
    c10::optional<torch::Tensor> vc) {
  check_bf16_cuda(qkv, "qkv");
  TORCH_CHECK(qkv.dim() == 3, "qkv must be [B, S, (H+2*Hkv)*D]");
  TORCH_CHECK(kc.has_value() == vc.has_value(),
              "give both caches or neither");
  const int64_t B = qkv.size(0), S = qkv.size(1), W = qkv.size(2);
  TORCH_CHECK(B > 0 && S > 0, "qkv must be non-empty");
  TORCH_CHECK(H > 0 && Hkv > 0 && W % (H + 2 * Hkv) == 0,
              "qkv width ", W, " is not (", H, "+2*", Hkv, ")*D");
  const int64_t D = W / (H + 2 * Hkv);
  TORCH_CHECK(D >= 8 && D % 8 == 0,
              "head dim must be a multiple of 8, got ", D);
  TORCH_CHECK(B * S <= std::numeric_limits<int>::max() &&
              W <= std::numeric_limits<int>::max(), "qkv too large");
  auto aligned = [](const torch::Tensor& t) {
    return reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0;
  };
  TORCH_CHECK(aligned(qkv), "qkv must be 16-byte aligned");
  for (const auto* t : {&cosT, &sinT}) {
    TORCH_CHECK(t->is_cuda() && t->device() == qkv.device() &&
                t->scalar_type() == torch::kFloat && t->is_contiguous() &&
                t->dim() == 2 && t->size(1) == D / 2 && aligned(*t),
                "rope tables must be contiguous 16-byte aligned f32 "
                "[rows, D/2] on qkv's device");
  }
  TORCH_CHECK(sinT.size(0) == cosT.size(0), "rope tables differ in rows");
  const int64_t rows = cosT.size(0);
  TORCH_CHECK(rows <= std::numeric_limits<int>::max(), "rope tables too long");
  TORCH_CHECK(pos0 >= 0, "pos0 must be >= 0, got ", pos0);
  TORCH_CHECK(pos0 + S <= rows, "positions ", pos0, " .. ", pos0 + S - 1,
              " exceed the ", rows, " rope table rows");
  auto q = torch::empty({B, S, H, D}, qkv.options());
  int64_t Bc = 0, Smax = 0;
  torch::Tensor k, v;
  if (kc.has_value()) {
    check_caches(*kc, *vc);
    TORCH_CHECK(kc->device() == qkv.device() && vc->device() == qkv.device(),
                "caches and qkv on different devices");
    TORCH_CHECK(kc->size(1) == Hkv && kc->size(3) == D,
                "caches must be [Bc, ", Hkv, ", Smax, ", D, "]");
    TORCH_CHECK(aligned(*kc) && aligned(*vc),
                "caches must be 16-byte aligned");
    Bc = kc->size(0);
    Smax = kc->size(2);
    TORCH_CHECK(Bc >= B, "cache has ", Bc, " batch rows for ", B);
    TORCH_CHECK(Smax > 0 && Smax <= std::numeric_limits<int>::max() &&
                pos0 + S <= Smax, "positions ", pos0, " .. ", pos0 + S - 1,
                " exceed the cache's ", Smax, " rows");
    k = *kc;
    v = *vc;
  } else {
    k = torch::empty({B, S, Hkv, D}, qkv.options());
    v = torch::empty({B, S, Hkv, D}, qkv.options());
  }
  check_hip(sentio_prefill_qkv_prep(
                qkv.data_ptr(), q.data_ptr(), k.data_ptr(), v.data_ptr(),
                cosT.data_ptr<float>(), sinT.data_ptr<float>(), (int)B, (int)S,
                (int)H, (int)Hkv, (int)D, (int)Bc, (int)Smax, (int)pos0,
                (int)rows, stream()), "prefill_qkv_prep");
  if (kc.has_value()) return {q};
  return {q, k, v};
}

torch::Tensor softmax_lastdim(torch::Tensor x) {
  check_bf16_cuda(x, "x");
  const int D = x.size(-1);
  auto y = torch::empty_like(x);
  check_hip(sentio_softmax(x.data_ptr(), y.data_ptr(), x.numel() / D, D,
                           stream()), "softmax");
  return y;
}

torch::Tensor mean_pool_l2norm(torch::Tensor hidden, torch::Tensor mask) {
  check_bf16_cuda(hidden, "hidden");
  TORCH_CHECK(hidden.dim() == 3, "hidden must be [B,S,D]");
  auto m = mask.to(torch::kUInt8).contiguous();
  auto out = torch::empty({hidden.size(0), hidden.size(2)},
                          hidden.options().dtype(torch::kFloat));
  check_hip(sentio_mean_pool_l2norm(hidden.data_ptr(), m.data_ptr<uint8_t>(),
                                    out.data_ptr<float>(), hidden.size(0),
                                    hidden.size(1), hidden.size(2), stream()),
            "mean_pool_l2norm");
  return out;
}

torch::Tensor sample_token(torch::Tensor logits, double temperature,
                           int64_t seed) {
  TORCH_CHECK(logits.is_cuda() && logits.dim() == 2, "logits must be [B,V] GPU");
  auto l = logits.to(torch::kFloat).contiguous();
  const long B = l.size(0);
  auto out = torch::empty({B}, l.options().dtype(torch::kLong));
  auto ws_val = torch::empty({B * 16}, l.options());
  auto ws_idx = torch::empty({B * 16}, l.options().dtype(torch::kInt));
  check_hip(sentio_sample(l.data_ptr<float>(), out.data_ptr<int64_t>(),
                          ws_val.data_ptr<float>(), ws_idx.data_ptr<int>(),
                          B, l.size(1), (float)temperature,
                          (unsigned)seed, stream()), "sample");
  return out;
}

// per-row sampling parameters: [B] tensors on the logits' device
torch::Tensor row_param(const torch::Tensor& t, const torch::Tensor& like,
                        torch::ScalarType dt, const char* name) {
  TORCH_CHECK(t.dim() == 1 && t.size(0) == like.size(0), name,
              " must be [B]");
  return t.to(like.device(), dt).contiguous();
}

std::vector<torch::Tensor> sample_support(torch::Tensor logits,
                                          torch::Tensor temperature,
                                          torch::Tensor top_k,
                                          torch::Tensor top_p) {
  TORCH_CHECK(logits.is_cuda() && logits.dim() == 2, "logits must be [B,V] GPU");
  auto l = logits.to(torch::kFloat).contiguous();
  const long B = l.size(0);
  TORCH_CHECK(B > 0 && l.size(1) > 0, "logits must be non-empty");
  auto t = row_param(temperature, l, torch::kFloat, "temperature");
  auto k = row_param(top_k, l, torch::kInt, "top_k");
  auto p = row_param(top_p, l, torch::kFloat, "top_p");
  auto tau = torch::empty({B}, l.options());
  auto count = torch::empty({B}, l.options().dtype(torch::kInt));
  check_hip(sentio_sample_support(l.data_ptr<float>(), t.data_ptr<float>(),
                                  k.data_ptr<int>(), p.data_ptr<float>(),
                                  tau.data_ptr<float>(), count.data_ptr<int>(),
                                  B, l.size(1), stream()), "sample_support");
  return {tau, count};
}

torch::Tensor sample_filtered(torch::Tensor logits, torch::Tensor temperature,
                              torch::Tensor top_k, torch::Tensor top_p,
                              torch::Tensor seed, torch::Tensor step) {
  TORCH_CHECK(logits.is_cuda() && logits.dim() == 2, "logits must be [B,V] GPU");
  auto l = logits.to(torch::kFloat).contiguous();
  const long B = l.size(0);
  TORCH_CHECK(B > 0 && l.size(1) > 0, "logits must be non-empty");
  auto t = row_param(temperature, l, torch::kFloat, "temperature");
  auto k = row_param(top_k, l, torch::kInt, "top_k");
  auto p = row_param(top_p, l, torch::kFloat, "top_p");
  auto sd = row_param(seed, l, torch::kLong, "seed");
  auto st = row_param(step, l, torch::kInt, "step");
  auto out = torch::empty({B}, l.options().dtype(torch::kLong));
  check_hip(sentio_sample_filtered(l.data_ptr<float>(), t.data_ptr<float>(),
                                   k.data_ptr<int>(), p.data_ptr<float>(),
                                   (const long*)sd.data_ptr<int64_t>(),
                                   st.data_ptr<int>(),
                                   (long*)out.data_ptr<int64_t>(), B,
                                   l.size(1), stream()), "sample_filtered");
  return out;
}

// In place on step and tok, so nothing here may convert or copy: every
// tensor must already have its kernel dtype and be contiguous on the GPU.
void sample_slots(torch::Tensor logits, c10::optional<torch::Tensor> slot,
                  torch::Tensor temperature, torch::Tensor top_k,
                  torch::Tensor top_p, torch::Tensor seed, torch::Tensor step,
                  c10::optional<torch::Tensor> active, torch::Tensor tok) {
  TORCH_CHECK(logits.is_cuda() && logits.dim() == 2 &&
              logits.scalar_type() == torch::kFloat && logits.is_contiguous(),
              "logits must be a contiguous f32 [R,V] GPU tensor");
  const long R = logits.size(0);
  const long S = tok.numel();
  TORCH_CHECK(R > 0 && S > 0 && logits.size(1) > 0,
              "logits and slots must be non-empty");
  auto slot_arr = [&](const torch::Tensor& t, torch::ScalarType dt, long n,
                      const char* name) {
    TORCH_CHECK(t.dim() == 1 && t.size(0) == n && t.scalar_type() == dt &&
                t.is_contiguous() && t.device() == logits.device(), name,
                " must be a contiguous [", n, "] tensor of its kernel dtype "
                "on the logits' device");
  };
  slot_arr(tok, torch::kLong, S, "tok");
  slot_arr(temperature, torch::kFloat, S, "temperature");
  slot_arr(top_k, torch::kInt, S, "top_k");
  slot_arr(top_p, torch::kFloat, S, "top_p");
  slot_arr(seed, torch::kLong, S, "seed");
  slot_arr(step, torch::kInt, S, "step");
  if (slot.has_value()) slot_arr(*slot, torch::kInt, R, "slot");
  else TORCH_CHECK(R == S, "without a slot table logits must be [S,V]");
  if (active.has_value()) slot_arr(*active, torch::kByte, S, "active");
  check_hip(sentio_sample_slots(
      logits.data_ptr<float>(),
      slot.has_value() ? slot->data_ptr<int>() : nullptr,
      temperature.data_ptr<float>(), top_k.data_ptr<int>(),
      top_p.data_ptr<float>(), (const long*)seed.data_ptr<int64_t>(),
      step.data_ptr<int>(),
      active.has_value() ? active->data_ptr<uint8_t>() : nullptr,
      (long*)tok.data_ptr<int64_t>(), R, (int)S, (int)logits.size(1),
      stream()), "sample_slots");
}

// The grammar tables of constrained sampling: next int16 [N, Vt], mask int32
// [N, ceil(Vt/32)], dist int16 [N], contiguous on the logits' device.
struct GrammarTables {
  int N, Vt, W;
};
GrammarTables check_tables(const torch::Tensor& next, const torch::Tensor& mask,
                           const torch::Tensor& dist, const torch::Tensor& like,
                           int64_t max_dist) {
  auto on = [&](const torch::Tensor& t, torch::ScalarType dt, int64_t dim,
                const char* name) {
    TORCH_CHECK(t.dim() == dim && t.scalar_type() == dt && t.is_contiguous() &&
                t.device() == like.device(), name, " must be a contiguous ",
                dim, "-d tensor of its kernel dtype on the logits' device");
  };
  on(next, torch::kShort, 2, "next");
  on(mask, torch::kInt, 2, "mask");
  on(dist, torch::kShort, 1, "dist");
  const int64_t N = next.size(0), Vt = next.size(1);
  TORCH_CHECK(N >= 1 && N <= 32767 && Vt >= 1, "next must be [N <= 32767, Vt]");
  TORCH_CHECK(mask.size(0) == N && mask.size(1) == (Vt + 31) / 32,
              "mask must be [N, ceil(Vt/32)]");
  TORCH_CHECK(mask.size(1) <= 2048, "at most 65536 tokenizer entries");
  TORCH_CHECK(dist.size(0) == N, "dist must be [N]");
  TORCH_CHECK(max_dist >= 0 && max_dist <= 32767, "bad max_dist");
  return {(int)N, (int)Vt, (int)mask.size(1)};
}

// In place on state and left (int32 [B]); returns tok [B] int64.
torch::Tensor sample_constrained(torch::Tensor logits,
                                 torch::Tensor temperature, torch::Tensor top_k,
                                 torch::Tensor top_p, torch::Tensor seed,
                                 torch::Tensor step, torch::Tensor state,
                                 torch::Tensor left, torch::Tensor next,
                                 torch::Tensor mask, torch::Tensor dist,
                                 int64_t max_dist) {
  TORCH_CHECK(logits.is_cuda() && logits.dim() == 2, "logits must be [B,V] GPU");
  auto l = logits.to(torch::kFloat).contiguous();
  const long B = l.size(0);
  TORCH_CHECK(B > 0 && l.size(1) > 0, "logits must be non-empty");
  auto t = row_param(temperature, l, torch::kFloat, "temperature");
  auto k = row_param(top_k, l, torch::kInt, "top_k");
  auto p = row_param(top_p, l, torch::kFloat, "top_p");
  auto sd = row_param(seed, l, torch::kLong, "seed");
  auto st = row_param(step, l, torch::kInt, "step");
  auto inplace = [&](const torch::Tensor& x, const char* name) {
    TORCH_CHECK(x.dim() == 1 && x.size(0) == B &&
                x.scalar_type() == torch::kInt && x.is_contiguous() &&
                x.device() == l.device(), name,
                " must be a contiguous int32 [B] tensor on the logits' device");
  };
  inplace(state, "state");
  inplace(left, "left");
  const GrammarTables g = check_tables(next, mask, dist, l, max_dist);
  auto out = torch::empty({B}, l.options().dtype(torch::kLong));
  check_hip(sentio_sample_constrained(
      l.data_ptr<float>(), t.data_ptr<float>(), k.data_ptr<int>(),
      p.data_ptr<float>(), (const long*)sd.data_ptr<int64_t>(),
      st.data_ptr<int>(), state.data_ptr<int>(), left.data_ptr<int>(),
      (const short*)next.data_ptr<int16_t>(), mask.data_ptr<int>(),
      (const short*)dist.data_ptr<int16_t>(), (long*)out.data_ptr<int64_t>(),
      B, (int)l.size(1), g.Vt, g.N, g.W, (int)max_dist, stream()),
      "sample_constrained");
  return out;
}

// sample_slots with per-slot automaton state: in place on step, tok, state
// and left, so nothing is converted or copied.
void sample_slots_constrained(
    torch::Tensor logits, c10::optional<torch::Tensor> slot,
    torch::Tensor temperature, torch::Tensor top_k, torch::Tensor top_p,
    torch::Tensor seed, torch::Tensor step,
    c10::optional<torch::Tensor> active, torch::Tensor tok,
    torch::Tensor state, torch::Tensor left, torch::Tensor next,
    torch::Tensor mask, torch::Tensor dist, int64_t max_dist) {
  TORCH_CHECK(logits.is_cuda() && logits.dim() == 2 &&
              logits.scalar_type() == torch::kFloat && logits.is_contiguous(),
              "logits must be a contiguous f32 [R,V] GPU tensor");
  const long R = logits.size(0);
  const long S = tok.numel();
  TORCH_CHECK(R > 0 && S > 0 && logits.size(1) > 0,
              "logits and slots must be non-empty");
  auto slot_arr = [&](const torch::Tensor& t, torch::ScalarType dt, long n,
                      const char* name) {
    TORCH_CHECK(t.dim() == 1 && t.size(0) == n && t.scalar_type() == dt &&
                t.is_contiguous() && t.device() == logits.device(), name,
                " must be a contiguous [", n, "] tensor of its kernel dtype "
                "on the logits' device");
  };
  slot_arr(tok, torch::kLong, S, "tok");
  slot_arr(temperature, torch::kFloat, S, "temperature");
  slot_arr(top_k, torch::kInt, S, "top_k");
  slot_arr(top_p, torch::kFloat, S, "top_p");
  slot_arr(seed, torch::kLong, S, "seed");
  slot_arr(step, torch::kInt, S, "step");
  slot_arr(state, torch::kInt, S, "state");
  slot_arr(left, torch::kInt, S, "left");
  if (slot.has_value()) slot_arr(*slot, torch::kInt, R, "slot");
  else TORCH_CHECK(R == S, "without a slot table logits must be [S,V]");
  if (active.has_value()) slot_arr(*active, torch::kByte, S, "active");
  const GrammarTables g = check_tables(next, mask, dist, logits, max_dist);
  check_hip(sentio_sample_slots_constrained(
      logits.data_ptr<float>(),
      slot.has_value() ? slot->data_ptr<int>() : nullptr,
      temperature.data_ptr<float>(), top_k.data_ptr<int>(),
      top_p.data_ptr<float>(), (const long*)seed.data_ptr<int64_t>(),
      step.data_ptr<int>(),
      active.has_value() ? active->data_ptr<uint8_t>() : nullptr,
      (long*)tok.data_ptr<int64_t>(), state.data_ptr<int>(),
      left.data_ptr<int>(), (const short*)next.data_ptr<int16_t>(),
      mask.data_ptr<int>(), (const short*)dist.data_ptr<int16_t>(), R, (int)S,
      (int)logits.size(1), g.Vt, g.N, g.W, (int)max_dist, stream()),
      "sample_slots_constrained");
}

torch::Tensor cosine_scores(torch::Tensor q, torch::Tensor mat) {
  TORCH_CHECK(q.is_cuda() && mat.is_cuda(), "must be on GPU");
  TORCH_CHECK(q.scalar_type() == mat.scalar_type(), "q/mat dtype mismatch");
  const long N = mat.size(0);
  const int D = mat.size(1);
  const int B = q.size(0);
  auto scores = torch::empty({B, N}, q.options().dtype(torch::kFloat));
  hipError_t e;
  if (q.scalar_type() == torch::kHalf)
    e = sentio_cosine_scores_f16(mat.data_ptr(), q.data_ptr(),
                                 scores.data_ptr<float>(), N, D, B, stream());
  else if (q.scalar_type() == torch::kBFloat16)
    e = sentio_cosine_scores_bf16(mat.data_ptr(), q.data_ptr(),
                                  scores.data_ptr<float>(), N, D, B, stream());
  else
    TORCH_CHECK(false, "cosine_scores expects fp16/bf16");
  check_hip(e, "cosine_scores");
  return scores;
}

torch::Tensor bm25_score(torch::Tensor term_ids, torch::Tensor indptr,
                         torch::Tensor post_doc, torch::Tensor post_tf,
                         torch::Tensor idf, torch::Tensor doc_len,
                         int64_t n_docs, double k1, double b, double avgdl,
                         double plus_delta) {
  auto scores = torch::zeros({n_docs}, post_tf.options().dtype(torch::kFloat));
  const int T = term_ids.size(0);
  if (T == 0) return scores;
  auto tids = term_ids.to(torch::kLong).contiguous();
  auto starts = indptr.index({tids});
  auto ends = indptr.index({tids + 1});
  auto lens = ends - starts;
  auto qoff = torch::zeros({T + 1}, tids.options());
  qoff.index_put_({torch::indexing::Slice(1, T + 1)}, torch::cumsum(lens, 0));
  const long total = qoff[-1].item<long>();
  if (total == 0) return scores;
  check_hip(sentio_bm25(tids.data_ptr<int64_t>(), qoff.data_ptr<int64_t>(),
                        starts.contiguous().data_ptr<int64_t>(),
                        post_doc.data_ptr<int>(), post_tf.data_ptr<float>(),
                        idf.data_ptr<float>(), doc_len.data_ptr<float>(),
                        scores.data_ptr<float>(), T, total, (float)k1,
                        (float)b, (float)avgdl, (float)plus_delta, stream()),
            "bm25");
  return scores;
}

torch::Tensor flash_attn(torch::Tensor q, torch::Tensor k, torch::Tensor v,
                         bool causal, double scale, torch::Tensor kv_lens) {
  check_bf16_cuda(q, "q");
  check_bf16_cuda(k, "k");
  check_bf16_cuda(v, "v");
  TORCH_CHECK(q.dim() == 4, "q must be [B,S,H,D]");
  const int B = q.size(0), S = q.size(1), H = q.size(2), D = q.size(3);
  const int Hkv = k.size(2);
  auto out = torch::empty_like(q);
  auto kl = kv_lens.to(torch::kInt).contiguous();
  check_hip(sentio_flash_attn(q.data_ptr(), k.data_ptr(), v.data_ptr(),
                              out.data_ptr(), kl.data_ptr<int>(), B, S, H,
                              Hkv, D, (float)scale, causal ? 1 : 0, stream()),
            "flash_attn");
  return out;
}

// Launch policy of the decode-attention kernel: (splits, waves per block).
// Once B*Hkv blocks fill the 256 CUs, one 8-wave block per (b, kv-head)
// streams the whole row and writes bf16 output itself: no workspace, no
// combine launch.  Below that, split-S across 4-wave blocks so the grid
// reaches >= 2 blocks per CU.  SENTIO_DECODE_SPLITS (clamped to one split
// per 256 cache rows) and SENTIO_DECODE_WAVES (4 or 8) override either
// half for probes and tests.
std::tuple<int, int> decode_attn_plan(long B, long Hkv, long Smax) {
  TORCH_CHECK(B > 0 && Hkv > 0 && Smax > 0, "decode_attn_plan: empty shape");
  const long blocks = B * Hkv;
  const int max_splits = (int)std::max(1L, Smax / 256);
  int splits = 1, waves = 8;
  if (blocks < 256) {
    splits = (int)std::max(1L, std::min((512 + blocks - 1) / blocks,
                                        (long)max_splits));
    waves = 4;
  }
  if (const char* ov = std::getenv("SENTIO_DECODE_SPLITS"))
    splits = std::max(1, std::min(atoi(ov), max_splits));
  if (const char* ov = std::getenv("SENTIO_DECODE_WAVES")) {
    waves = atoi(ov);
    TORCH_CHECK(waves == 4 || waves == 8,
                "SENTIO_DECODE_WAVES must be 4 or 8, got '", ov, "'");
  }
  return {splits, waves};
}

// fp32 split-S partials; empty when the decode kernel writes `out` itself
struct DecodeWorkspace {
  torch::Tensor o, ml;
  float* o_ptr = nullptr;
  float* ml_ptr = nullptr;
  DecodeWorkspace(const torch::Tensor& like, int splits, long B, long Hkv,
                  long G, long D) {
    if (splits <= 1) return;
    const long n = B * Hkv * splits * G;
    o = torch::empty({n * D}, like.options().dtype(torch::kFloat));
    ml = torch::empty({n * 2}, like.options().dtype(torch::kFloat));
    o_ptr = o.data_ptr<float>();
    ml_ptr = ml.data_ptr<float>();
  }
};

void check_caches(const torch::Tensor& kc, const torch::Tensor& vc) {
  check_bf16_cuda(kc, "k cache");
  check_bf16_cuda(vc, "v cache");
  TORCH_CHECK(kc.dim() == 4, "k cache must be [B,Hkv,Smax,D]");
  TORCH_CHECK(vc.sizes() == kc.sizes(), "k and v cache shapes differ");
}

torch::Tensor decode_attn(torch::Tensor q, torch::Tensor kc, torch::Tensor vc,
                          torch::Tensor seq_lens, double scale) {
  check_bf16_cuda(q, "q");
  TORCH_CHECK(q.dim() == 3, "q must be [B,H,D]");
  check_caches(kc, vc);
  const int B = q.size(0), H = q.size(1), D = q.size(2);
  const int Hkv = kc.size(1), Smax = kc.size(2);
  TORCH_CHECK(kc.size(0) >= B && kc.size(3) == D, "cache/q shape mismatch");
  auto out = torch::empty_like(q);
  auto sl = seq_lens.to(torch::kInt).contiguous();
  const auto [splits, waves] = decode_attn_plan(B, Hkv, Smax);
  DecodeWorkspace ws(q, splits, B, Hkv, H / Hkv, D);
  check_hip(sentio_decode_attn(q.data_ptr(), kc.data_ptr(), vc.data_ptr(),
                               out.data_ptr(), sl.data_ptr<int>(), ws.o_ptr,
                               ws.ml_ptr, splits, waves, B, H, Hkv, Smax, D,
                               (float)scale, stream()), "decode_attn");
  return out;
}

// Decode attention with decode_qkv_prep folded in: RoPE(q) stays in
// registers, the new k/v row is written at seq_lens[b] and attended from
// registers; covers seq_lens[b] + 1 keys.
torch::Tensor decode_attn_fused(torch::Tensor qkv, torch::Tensor kc,
                                torch::Tensor vc, torch::Tensor cosT,
                                torch::Tensor sinT, torch::Tensor seq_lens,
                                double scale) {
  check_bf16_cuda(qkv, "qkv");
  TORCH_CHECK(qkv.dim() == 2, "qkv must be [B, (H+2*Hkv)*D]");
  check_caches(kc, vc);
  TORCH_CHECK(seq_lens.is_cuda() && seq_lens.scalar_type() == torch::kInt &&
              seq_lens.is_contiguous(),
              "seq_lens must be a contiguous i32 GPU tensor");
  const int B = qkv.size(0);
  const int Hkv = kc.size(1), Smax = kc.size(2), D = kc.size(3);
  TORCH_CHECK(D == 64 || D == 128, "head dim must be 64 or 128, got ", D);
  const int H = (int)(qkv.size(1) / D) - 2 * Hkv;
  TORCH_CHECK(H > 0 && H % Hkv == 0 &&
              (long)(H + 2 * Hkv) * D == qkv.size(1), "qkv width mismatch");
  TORCH_CHECK(kc.size(0) >= B && seq_lens.numel() == B,
              "batch mismatch between qkv, caches and seq_lens");
  for (const auto* t : {&cosT, &sinT}) {
    TORCH_CHECK(t->is_cuda() && t->scalar_type() == torch::kFloat &&
                t->is_contiguous() && t->dim() == 2 && t->size(0) >= Smax &&
                t->size(1) == D / 2,
                "rope tables must be contiguous f32 [>=Smax, D/2] on GPU");
  }
  auto out = torch::empty({B, H, D}, qkv.options());
  const auto [splits, waves] = decode_attn_plan(B, Hkv, Smax);
  DecodeWorkspace ws(qkv, splits, B, Hkv, H / Hkv, D);
  check_hip(sentio_decode_attn_fused(
                qkv.data_ptr(), kc.data_ptr(), vc.data_ptr(), out.data_ptr(),
                cosT.data_ptr<float>(), sinT.data_ptr<float>(),
                seq_lens.data_ptr<int>(), ws.o_ptr, ws.ml_ptr, splits, waves,
                B, H, Hkv, Smax, D, (float)scale, stream()),
            "decode_attn_fused");
  return out;
}

// ---- FP8 (e4m3fn) KV cache: uint8 caches + fp32 [Hkv] scales
void check_caches_u8(const torch::Tensor& kc, const torch::Tensor& vc) {
  for (const auto* t : {&kc, &vc}) {
    TORCH_CHECK(t->is_cuda() && t->scalar_type() == torch::kByte &&
                t->is_contiguous(),
                "fp8 caches must be contiguous uint8 GPU tensors");
  }
  TORCH_CHECK(kc.dim() == 4, "k cache must be [B,Hkv,Smax,D]");
  TORCH_CHECK(vc.sizes() == kc.sizes(), "k and v cache shapes differ");
}

void check_kv_scale(const torch::Tensor& t, const torch::Tensor& like,
                    long Hkv, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.device() == like.device() &&
              t.scalar_type() == torch::kFloat && t.is_contiguous() &&
              t.dim() == 1 && t.size(0) == Hkv,
              name, ": kv scale must be a contiguous f32 [Hkv] tensor on the "
              "caches' device");
}

// decode_attn_fused over an FP8 cache: the new k/v row is quantised with
// k_inv/v_inv and attended as its dequantised stored value.
torch::Tensor decode_attn_fused_fp8(torch::Tensor qkv, torch::Tensor kc,
                                    torch::Tensor vc, torch::Tensor cosT,
                                    torch::Tensor sinT, torch::Tensor seq_lens,
                                    torch::Tensor k_scale,
                                    torch::Tensor v_scale, torch::Tensor k_inv,
                                    torch::Tensor v_inv, double scale) {
  check_bf16_cuda(qkv, "qkv");
  TORCH_CHECK(qkv.dim() == 2, "qkv must be [B, (H+2*Hkv)*D]");
  check_caches_u8(kc, vc);
  TORCH_CHECK(seq_lens.is_cuda() && seq_lens.scalar_type() == torch::kInt &&
              seq_lens.is_contiguous(),
              "seq_lens must be a contiguous i32 GPU tensor");
  const int B = qkv.size(0);
  const int Hkv = kc.size(1), Smax = kc.size(2), D = kc.size(3);
  TORCH_CHECK(D == 64 || D == 128, "head dim must be 64 or 128, got ", D);
  const int H = (int)(qkv.size(1) / D) - 2 * Hkv;
  TORCH_CHECK(H > 0 && H % Hkv == 0 &&
              (long)(H + 2 * Hkv) * D == qkv.size(1), "qkv width mismatch");
  TORCH_CHECK(H / Hkv <= 8, "at most 8 query heads per kv head, got ",
              H / Hkv);
  TORCH_CHECK(kc.size(0) >= B && seq_lens.numel() == B,
              "batch mismatch between qkv, caches and seq_lens");
  for (const auto* t : {&cosT, &sinT}) {
    TORCH_CHECK(t->is_cuda() && t->scalar_type() == torch::kFloat &&
                t->is_contiguous() && t->dim() == 2 && t->size(0) >= Smax &&
                t->size(1) == D / 2,
                "rope tables must be contiguous f32 [>=Smax, D/2] on GPU");
  }
  check_kv_scale(k_scale, kc, Hkv, "k_scale");
  check_kv_scale(v_scale, kc, Hkv, "v_scale");
  check_kv_scale(k_inv, kc, Hkv, "k_inv");
  check_kv_scale(v_inv, kc, Hkv, "v_inv");
  auto out = torch::empty({B, H, D}, qkv.options());
  const auto [splits, waves] = decode_attn_plan(B, Hkv, Smax);
  DecodeWorkspace ws(qkv, splits, B, Hkv, H / Hkv, D);
  check_hip(sentio_decode_attn_fused_fp8(
                qkv.data_ptr(), kc.data_ptr(), vc.data_ptr(), out.data_ptr(),
                cosT.data_ptr<float>(), sinT.data_ptr<float>(),
                seq_lens.data_ptr<int>(), k_scale.data_ptr<float>(),
                v_scale.data_ptr<float>(), k_inv.data_ptr<float>(),
                v_inv.data_ptr<float>(), ws.o_ptr, ws.ml_ptr, splits, waves,
                B, H, Hkv, Smax, D, (float)scale, stream()),
            "decode_attn_fused_fp8");
  return out;
}

// Quantising splice of bf16 staging K/V [n,Hkv,S_src,D] into rows[i] of the
// uint8 caches, first S sequence rows.
void kv_store_fp8(torch::Tensor src_k, torch::Tensor src_v, torch::Tensor kc,
                  torch::Tensor vc, torch::Tensor rows, long S,
                  torch::Tensor k_inv, torch::Tensor v_inv) {
  check_bf16_cuda(src_k, "src_k");
  check_bf16_cuda(src_v, "src_v");
  TORCH_CHECK(src_k.dim() == 4 && src_v.sizes() == src_k.sizes(),
              "sources must be two [n,Hkv,S_src,D] tensors of equal shape");
  check_caches_u8(kc, vc);
  const long n = src_k.size(0), Hkv = kc.size(1), Smax = kc.size(2);
  const long D = kc.size(3), S_src = src_k.size(2);
  TORCH_CHECK(src_k.size(1) == Hkv && src_k.size(3) == D,
              "source and cache kv heads / head dim differ");
  TORCH_CHECK(D % 8 == 0, "head dim must be a multiple of 8, got ", D);
  TORCH_CHECK(S >= 0 && S <= S_src && S <= Smax,
              "S must be <= min(S_src, Smax), got ", S);
  TORCH_CHECK(rows.is_cuda() && rows.device() == kc.device() &&
              rows.scalar_type() == torch::kInt && rows.is_contiguous() &&
              rows.dim() == 1 && rows.numel() == n,
              "rows must be a contiguous i32 [n] tensor on the caches' device");
  TORCH_CHECK(src_k.device() == kc.device(), "sources and caches on "
              "different devices");
  check_kv_scale(k_inv, kc, Hkv, "k_inv");
  check_kv_scale(v_inv, kc, Hkv, "v_inv");
  check_hip(sentio_kv_store_fp8(
                src_k.data_ptr(), src_v.data_ptr(), kc.data_ptr(),
                vc.data_ptr(), rows.data_ptr<int>(), k_inv.data_ptr<float>(),
                v_inv.data_ptr<float>(), (int)n, (int)kc.size(0), (int)Hkv,
                (int)S_src, (int)S, (int)Smax, (int)D, stream()),
            "kv_store_fp8");
}

// Launch policy of the split-K decode GEMM: (S, blocks, slab bytes) for
// x [M, K] @ W[N, K]^T.  S = 0 means no plan: the kernel does not take the
// shape (M > 32, N not a multiple of its 64-column tile, K not a multiple
// of its 32-deep k-step) or no legal S reaches 128 blocks within 8 MB of
// slabs, and the caller keeps the library GEMM.  Blocks = (N / 64) * S
// should land in 256..512, one to two 8-wave blocks per CU; among those a
// slice K / S of whole 512-deep chunks (8 weight loads per wave in flight,
// twice) beats whole 256-deep ones, and then the smallest S wins: fewer
// slab bytes for the norm kernel to sum (measured on llama3-8b: S = 4 for
// both wo and down; profiles/decode_gemm_splitk.md).  SENTIO_GEMM_SPLITK
// overrides S for shapes the kernel takes, for probes and tests.
std::tuple<int, long, long> decode_gemm_plan(long M, long N, long K) {
  TORCH_CHECK(M > 0 && N > 0 && K > 0, "decode_gemm_plan: empty shape");
  if (M > 32 || N % 64 || K % 32) return {0, 0, 0};
  const long tiles = N / 64;
  auto slab_bytes = [&](long s) { return s * M * N * 4; };
  if (const char* ov = std::getenv("SENTIO_GEMM_SPLITK")) {
    const long s = atol(ov);
    TORCH_CHECK(s >= 1 && s <= 65535 && K % (32 * s) == 0,
                "SENTIO_GEMM_SPLITK='", ov, "' does not split K=", K,
                " into slices that are multiples of 32");
    return {(int)s, tiles * s, slab_bytes(s)};
  }
  long best = 0, best_pen = 0, best_depth = 0;
  for (long s = 1; s <= K / 32; ++s) {
    if (K % (32 * s) || slab_bytes(s) > (8L << 20)) continue;
    const long blocks = tiles * s, slice = K / s;
    if (blocks < 128) continue;
    const long pen = blocks < 256 ? 256 - blocks
                   : blocks > 512 ? blocks - 512 : 0;
    const long depth = slice % 512 == 0 ? 2 : slice % 256 == 0 ? 1 : 0;
    if (!best || pen < best_pen || (pen == best_pen && depth > best_depth)) {
      best = s; best_pen = pen; best_depth = depth;
    }
  }
  if (!best) return {0, 0, 0};
  return {(int)best, tiles * best, slab_bytes(best)};
}

// Split-K partials of x [M, K] @ w[N, K]^T as fp32 [S, M, N]; S from
// decode_gemm_plan.  nan_fill (tests) pre-fills the slabs with NaN so that
// an element the kernel does not write stays visible.
torch::Tensor decode_gemm_splitk(torch::Tensor x, torch::Tensor w,
                                 bool nan_fill) {
  check_bf16_cuda(x, "x");
  check_bf16_cuda(w, "w");
  TORCH_CHECK(x.dim() == 2 && w.dim() == 2 && x.size(1) == w.size(1),
              "x [M,K], w [N,K]");
  const long M = x.size(0), K = x.size(1), N = w.size(0);
  const int S = std::get<0>(decode_gemm_plan(M, N, K));
  TORCH_CHECK(S > 0, "decode_gemm_splitk: no plan for M=", M, " N=", N,
              " K=", K, " (use the library GEMM)");
  auto opts = x.options().dtype(torch::kFloat);
  auto part = nan_fill
      ? torch::full({S, M, N}, std::numeric_limits<float>::quiet_NaN(), opts)
      : torch::empty({S, M, N}, opts);
  check_hip(sentio_decode_gemm_splitk(x.data_ptr(), w.data_ptr(),
                                      part.data_ptr<float>(), (int)M, (int)K,
                                      (int)N, S, stream()),
            "decode_gemm_splitk");
  return part;
}

// reread: take the kernel that loads h back from memory at any row length
// (tests compare the register path against it)
std::vector<torch::Tensor> rmsnorm_residual_partials(torch::Tensor part,
                                                     torch::Tensor res,
                                                     torch::Tensor w,
                                                     double eps, bool reread) {
  TORCH_CHECK(part.is_cuda() && part.scalar_type() == torch::kFloat &&
              part.is_contiguous() && part.dim() >= 2,
              "part must be a contiguous f32 [S, ..., D] GPU tensor");
  check_bf16_cuda(res, "res");
  check_bf16_cuda(w, "w");
  const int S = part.size(0);
  const int D = part.size(-1);
  TORCH_CHECK(S >= 1 && res.numel() * S == part.numel() && res.size(-1) == D &&
              w.numel() == D, "part [S, rows, D], res [rows, D], w [D]");
  const long rows = res.numel() / D;
  auto y = torch::empty_like(res);
  auto h = torch::empty_like(res);
  check_hip(sentio_rmsnorm_residual_partials(
                part.data_ptr<float>(), res.data_ptr(), w.data_ptr(),
                y.data_ptr(), h.data_ptr(), S, rows, D, (float)eps,
                reread ? 1 : 0, stream()),
            "rmsnorm_residual_partials");
  return {y, h};
}

torch::Tensor gemm_bf16(torch::Tensor a, torch::Tensor b) {
  check_bf16_cuda(a, "a");
  check_bf16_cuda(b, "b");
  const int M = a.size(0), K = a.size(1), N = b.size(1);
  TORCH_CHECK(b.size(0) == K, "inner dims mismatch");
  auto c = torch::empty({M, N}, a.options());
  check_hip(sentio_gemm_bf16(a.data_ptr(), b.data_ptr(), c.data_ptr(), M, N, K,
                             stream()), "gemm_bf16");
  return c;
}

}  // namespace

torch::Tensor skinny_gemm(torch::Tensor x, torch::Tensor w) {
  check_bf16_cuda(x, "x");
  check_bf16_cuda(w, "w");
  TORCH_CHECK(x.dim() == 2 && w.dim() == 2, "x [M,K], w [N,K]");
  TORCH_CHECK(x.size(1) == w.size(1), "K mismatch");
  const int M = x.size(0), K = x.size(1), N = w.size(0);
  auto out = torch::empty({M, N}, x.options());
  check_hip(sentio_skinny_gemm(x.data_ptr(), w.data_ptr(), out.data_ptr(),
                               M, K, N, stream()), "skinny_gemm");
  return out;
}

std::vector<torch::Tensor> fuse_topk(torch::Tensor d_ids, torch::Tensor d_scores,
                                     torch::Tensor s_ids, torch::Tensor s_scores,
                                     int64_t top_k, int64_t method,
                                     double rrf_k, double dw, double sw) {
  TORCH_CHECK(d_ids.is_cuda() && d_ids.scalar_type() == torch::kLong, "d_ids i64 GPU");
  TORCH_CHECK(s_ids.scalar_type() == torch::kLong, "s_ids i64");
  const int B = d_ids.size(0), Kd = d_ids.size(1), Ks = s_ids.size(1);
  auto out_ids = torch::empty({B, top_k}, d_ids.options());
  auto out_scores = torch::empty({B, top_k},
                                 d_scores.options().dtype(torch::kFloat));
  check_hip(sentio_fuse_topk(
      d_ids.contiguous().data_ptr<int64_t>(),
      d_scores.to(torch::kFloat).contiguous().data_ptr<float>(),
      s_ids.contiguous().data_ptr<int64_t>(),
      s_scores.to(torch::kFloat).contiguous().data_ptr<float>(),
      out_ids.data_ptr<int64_t>(), out_scores.data_ptr<float>(), B, Kd, Ks,
      (int)top_k, (int)method, (float)rrf_k, (float)dw, (float)sw,
      stream()), "fuse_topk");
  return {out_ids, out_scores};
}

torch::Tensor lt_gemm_tn(torch::Tensor x, torch::Tensor w) {
  check_bf16_cuda(x, "x");
  check_bf16_cuda(w, "w");
  TORCH_CHECK(x.dim() == 2 && w.dim() == 2 && x.size(1) == w.size(1),
              "x [M,K], w [N,K]");
  const int M = x.size(0), K = x.size(1), N = w.size(0);
  auto out = torch::empty({M, N}, x.options());
  int rc = sentio_lt_gemm_tn(x.data_ptr(), w.data_ptr(), out.data_ptr(), M, N,
                             K, stream());
  TORCH_CHECK(rc == 0, "sentio_lt_gemm_tn failed rc=", rc);
  return out;
}

torch::Tensor flash_attn_cache(torch::Tensor q, torch::Tensor kc,
                               torch::Tensor vc, torch::Tensor kv_lens,
                               double scale, int64_t q_off) {
  check_bf16_cuda(q, "q");
  TORCH_CHECK(q.dim() == 4, "q must be [B,S,H,D] (suffix)");
  TORCH_CHECK(kc.dim() == 4 && vc.dim() == 4, "caches must be [B,Hkv,Smax,D]");
  TORCH_CHECK(kv_lens.scalar_type() == torch::kInt, "kv_lens must be i32");
  const int B = q.size(0), S = q.size(1), H = q.size(2), D = q.size(3);
  const int Hkv = kc.size(1), Smax = kc.size(2);
  auto out = torch::empty_like(q);
  check_hip(sentio_flash_attn_cache(q.data_ptr(), kc.data_ptr(), vc.data_ptr(),
                                    out.data_ptr(),
                                    kv_lens.contiguous().data_ptr<int>(), B, S,
                                    H, Hkv, Smax, D, (float)scale, (int)q_off,
                                    stream()), "flash_attn_cache");
  return out;
}

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("rmsnorm", &rmsnorm);
  m.def("rmsnorm_residual", &rmsnorm_residual);
  m.def("swiglu", &swiglu);
  m.def("swiglu_packed", &swiglu_packed);
  m.def("rope_apply", &rope_apply);
  m.def("decode_qkv_prep", &decode_qkv_prep);
  m.def("prefill_qkv_prep", &prefill_qkv_prep);
  m.def("softmax_lastdim", &softmax_lastdim);
  m.def("mean_pool_l2norm", &mean_pool_l2norm);
  m.def("sample_token", &sample_token);
  m.def("sample_support", &sample_support);
  m.def("sample_filtered", &sample_filtered);
  m.def("sample_slots", &sample_slots);
  m.def("sample_constrained", &sample_constrained);
  m.def("sample_slots_constrained", &sample_slots_constrained);
  m.def("cosine_scores", &cosine_scores);
  m.def("bm25_score", &bm25_score);
  m.def("flash_attn", &flash_attn);
  m.def("flash_attn_cache", &flash_attn_cache);
  m.def("decode_attn", &decode_attn);
  m.def("decode_attn_fused", &decode_attn_fused);
  m.def("decode_attn_fused_fp8", &decode_attn_fused_fp8);
  m.def("kv_store_fp8", &kv_store_fp8);
  m.def("decode_attn_plan", &decode_attn_plan);
  m.def("decode_gemm_plan", &decode_gemm_plan);
  m.def("decode_gemm_splitk", &decode_gemm_splitk);
  m.def("rmsnorm_residual_partials", &rmsnorm_residual_partials,
        py::arg("part"), py::arg("res"), py::arg("w"), py::arg("eps"),
        py::arg("reread") = false);
  m.def("gemm_bf16", &gemm_bf16);
  m.def("skinny_gemm", &skinny_gemm);
  m.def("fuse_topk", &fuse_topk);
  m.def("lt_gemm_tn", &lt_gemm_tn);
}
