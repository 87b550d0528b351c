// torch.ops.imgcomp.* — the conv / transposed-conv / GDN launchers of libimgcomp.so
// registered as PyTorch operators (TORCH_LIBRARY), so the autograd Functions in
// image_compression_amd/functional.py dispatch through the PyTorch op registry
// instead of ctypes, and FX / fake-tensor tracing sees real operators with
// shape (Meta) kernels.  Each op is one C-ABI call of include/imgcomp.h on the
// current HIP stream of the input's device, with its workspace from PyTorch's
// caching allocator; the C ABI stays the non-torch binding.
//
// Reference interfaces these replace: torch.nn.Conv2d in modelling/blocks/analysis.py:55 and
// prior_analysis.py:54-56; torch.nn.ConvTranspose2d in modelling/blocks/synthesis.py:55-57 and
// prior_synthesis.py:54-56; GDN.forward in modelling/layers/gdn.py:79-88 (backward by autograd there).
#include <ATen/ATen.h>
#include <ATen/hip/impl/HIPGuardImplMasqueradingAsCUDA.h>
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>
#include <torch/library.h>

#include <climits>
#include <tuple>

#include "../../include/imgcomp.h"

namespace {

using at::Tensor;

void check_operand(const Tensor& t, const char* what) {
  TORCH_CHECK(t.is_cuda(), "imgcomp: ", what, " must be on a ROCm device, got ", t.device());
  TORCH_CHECK(t.scalar_type() == at::kFloat, "imgcomp: ", what, " must be float32, got ", t.scalar_type());
}

ic_act act_of(const Tensor& t) {
  TORCH_CHECK(t.dim() == 4, "imgcomp: expected a 4-D tensor, got ", t.sizes());
  ic_act a;
  a.data = t.data_ptr<float>();
  a.n = (int)t.size(0); a.c = (int)t.size(1); a.h = (int)t.size(2); a.w = (int)t.size(3);
  a.sn = t.stride(0); a.sc = t.stride(1); a.sh = t.stride(2); a.sw = t.stride(3);
  return a;
}

// activations with >= 32 channels live channels-last (NHWC): GEMM operand rows are channel-contiguous
at::MemoryFormat act_format(int64_t c) { return c >= 32 ? at::MemoryFormat::ChannelsLast : at::MemoryFormat::Contiguous; }

Tensor new_act(const Tensor& like, int64_t n, int64_t c, int64_t h, int64_t w) {
  return at::empty({n, c, h, w}, like.options().memory_format(act_format(c)));
}

// PyTorch-ROCm exposes HIP devices under the "cuda" device type; these are its HIP stream / guard APIs for them
void* stream_of(const Tensor& t) {
  return (void*)c10::hip::getCurrentHIPStreamMasqueradingAsCUDA(t.device().index()).stream();
}

Tensor workspace(const Tensor& like, size_t nbytes) {
  return at::empty({(int64_t)std::max<size_t>(nbytes, 16)}, like.options().dtype(at::kByte));
}

void check_rc(int rc, const char* what) {
  TORCH_CHECK(rc == 0, "imgcomp: ", what, " failed with status ", rc,
              rc == IC_ERR_ARG ? " (unsupported/inconsistent arguments)"
                               : rc == IC_ERR_WORKSPACE ? " (workspace too small)" : " (HIP error)");
}

float* opt_ptr(const c10::optional<Tensor>& t) { return t.has_value() && t->defined() ? t->data_ptr<float>() : nullptr; }

// ---------------------------------------------------------------- conv2d / conv_transpose2d
// One launcher per op family (forward, input gradient, weight gradient), each for both kinds of conv (TR: the
// transposed one, weight [Cin][Cout][k][k]; else [Cout][Cin][k][k]); the registered ops below are bindings of
// them.  A family's *_out function allocates its outputs, for the launcher and for the op's shape (Meta) kernel.
// What a binding chooses: a bf16 copy of an operand (include/imgcomp.h *_xb; none: nullptr), a caller-owned
// workspace (the forwards; none: nullptr), and its own name for the messages.
template <bool TR>
Tensor conv_fwd_out(const Tensor& x, const Tensor& w, int64_t stride, int64_t pad, int64_t opad) {
  const int64_t k = w.size(2);
  const int64_t ho = TR ? (x.size(2) - 1) * stride - 2 * pad + k + opad : (x.size(2) + 2 * pad - k) / stride + 1;
  const int64_t wo = TR ? (x.size(3) - 1) * stride - 2 * pad + k + opad : (x.size(3) + 2 * pad - k) / stride + 1;
  return new_act(x, x.size(0), w.size(TR ? 1 : 0), ho, wo);
}

// dx has x's shape; its memory format is x's (like_x) or the one of its channel count (act_format)
Tensor conv_dgrad_out(const Tensor& dy, const Tensor& x, bool like_x) {
  return at::empty(x.sizes(), dy.options().memory_format(like_x ? x.suggest_memory_format() : act_format(x.size(1))));
}

// (dw, db); db is empty when bias is false
template <bool TR>
std::tuple<Tensor, Tensor> conv_wgrad_out(const Tensor& w, bool bias) {
  Tensor dw = at::empty_like(w, at::MemoryFormat::Contiguous);
  return {dw, at::empty({bias ? w.size(TR ? 1 : 0) : 0}, w.options())};
}

// x is the conv's input; dy (the gradients) its output gradient
template <bool TR>
void check_weight(const Tensor& w, const Tensor& x, const Tensor* dy = nullptr) {
  TORCH_CHECK(w.dim() == 4 && w.size(TR ? 0 : 1) == x.size(1) && w.size(2) == w.size(3),
              TR ? "conv_transpose2d: weight " : "conv2d: weight ", w.sizes(), " does not match input ", x.sizes());
  TORCH_CHECK(!dy || (dy->dim() == 4 && dy->size(1) == w.size(TR ? 1 : 0)),
              TR ? "conv_transpose2d: weight " : "conv2d: weight ", w.sizes(), " does not match the output gradient");
}

void check_copy(const Tensor& b, const Tensor& like, const char* what) {
  TORCH_CHECK(b.is_cuda() && b.scalar_type() == at::kBFloat16 && b.sizes() == like.sizes() &&
                  b.strides() == like.strides(),
              "imgcomp: ", what, " must be a bf16 tensor with the shape and strides of its fp32 tensor");
}

// A caller-owned workspace that persists across calls (eval-mode weight caching, functional._cached_conv) is
// grown here when too small (only on a packing call — with IC_MATH_WPACKED the pack must already be in it, so a
// short workspace is an error).
void ensure_ws(Tensor& ws, size_t nb, int64_t math, const char* what) {
  if ((size_t)ws.numel() >= nb) return;
  TORCH_CHECK(!(math & IC_MATH_WPACKED), "imgcomp: ", what, ": IC_MATH_WPACKED with a workspace of ", ws.numel(),
              " bytes, the op needs ", nb);
  ws.resize_({(int64_t)nb});
}

template <bool TR>
Tensor conv_fwd(const char* what, const Tensor& x, const Tensor* xb, const Tensor& w, const c10::optional<Tensor>& b,
                int64_t stride, int64_t pad, int64_t opad, int64_t act, int64_t math, Tensor* own_ws) {
  check_operand(x, "x");
  check_operand(w, "weight");
  if (b.has_value()) check_operand(*b, "bias");
  if (xb) check_copy(*xb, x, "xb");
  TORCH_CHECK(!own_ws || (own_ws->device() == x.device() && own_ws->scalar_type() == at::kByte && own_ws->dim() == 1 &&
                          own_ws->is_contiguous()),
              what, ": the workspace must be a contiguous uint8 vector on the input's device");
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(x.device());
  check_weight<TR>(w, x);
  Tensor y = conv_fwd_out<TR>(x, w, stride, pad, opad);
  const ic_act ax = act_of(x), ay = act_of(y);
  const int k = (int)w.size(2);
  // the query: with the copy's tiles; of a packing call, whether or not this call packs
  const int qmath = own_ws ? (int)(math & ~IC_MATH_WPACKED) : xb ? (int)math | IC_MATH_XB : (int)math;
  const size_t nb = (TR ? ic_conv_transpose2d_fwd_ws_ex : ic_conv2d_fwd_ws_ex)(&ax, k, (int)stride, (int)pad, &ay, qmath);
  Tensor tmp;
  if (own_ws) ensure_ws(*own_ws, nb, math, what);
  else tmp = workspace(x, nb);
  void* ws = own_ws ? own_ws->data_ptr() : tmp.data_ptr();
  const size_t ws_bytes = own_ws ? (size_t)own_ws->numel() : nb;
  check_rc(xb ? (TR ? ic_conv_transpose2d_fwd_xb : ic_conv2d_fwd_xb)(&ax, xb->data_ptr(), w.data_ptr<float>(), opt_ptr(b),
                                                                    k, (int)stride, (int)pad, &ay, (int)act, (int)math,
                                                                    ws, ws_bytes, stream_of(x))
              : (TR ? ic_conv_transpose2d_fwd_ex : ic_conv2d_fwd_ex)(&ax, w.data_ptr<float>(), opt_ptr(b), k, (int)stride,
                                                                    (int)pad, &ay, (int)act, (int)math, ws, ws_bytes,
                                                                    stream_of(x)),
           what);
  return y;
}

// x: the conv's input, read for its shape and memory format only
template <bool TR>
Tensor conv_dgrad(const char* what, const Tensor& dy, const Tensor* dyb, const Tensor& w, const Tensor& x, int64_t stride,
                  int64_t pad, int64_t math, bool like_x) {
  check_operand(dy, "dy");
  check_operand(w, "weight");
  if (dyb) check_copy(*dyb, dy, "dyb");
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(dy.device());
  check_weight<TR>(w, x, &dy);
  Tensor dx = conv_dgrad_out(dy, x, like_x);
  const ic_act ag = act_of(dy), adx = act_of(dx);
  const int k = (int)w.size(2);
  const size_t nb = (TR ? ic_conv_transpose2d_dgrad_ws_ex : ic_conv2d_dgrad_ws_ex)(&ag, k, (int)stride, (int)pad, &adx,
                                                                                   dyb ? (int)math | IC_MATH_XB : (int)math);
  Tensor ws = workspace(dy, nb);
  check_rc(dyb ? (TR ? ic_conv_transpose2d_dgrad_xb : ic_conv2d_dgrad_xb)(&ag, dyb->data_ptr(), w.data_ptr<float>(), k,
                                                                         (int)stride, (int)pad, &adx, (int)math,
                                                                         ws.data_ptr(), nb, stream_of(dy))
               : (TR ? ic_conv_transpose2d_dgrad_ex : ic_conv2d_dgrad_ex)(&ag, w.data_ptr<float>(), k, (int)stride, (int)pad,
                                                                         &adx, (int)math, ws.data_ptr(), nb, stream_of(dy)),
           what);
  return dx;
}

// xb and dyb: both or neither.  w is read for its shape only.
template <bool TR>
std::tuple<Tensor, Tensor> conv_wgrad(const char* what, const Tensor& x, const Tensor* xb, const Tensor& dy,
                                      const Tensor* dyb, const Tensor& w, int64_t stride, int64_t pad, bool bias,
                                      int64_t math) {
  check_operand(x, "x");
  check_operand(dy, "dy");
  check_operand(w, "weight");
  if (xb) check_copy(*xb, x, "xb");
  if (dyb) check_copy(*dyb, dy, "dyb");
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(dy.device());
  check_weight<TR>(w, x, &dy);
  std::tuple<Tensor, Tensor> out = conv_wgrad_out<TR>(w, bias);
  float* dw = std::get<0>(out).data_ptr<float>();
  float* db = bias ? std::get<1>(out).data_ptr<float>() : nullptr;
  const ic_act ax = act_of(x), ag = act_of(dy);
  const int k = (int)w.size(2);
  const size_t nb = (TR ? ic_conv_transpose2d_wgrad_ws_ex : ic_conv2d_wgrad_ws_ex)(&ax, &ag, k, (int)stride, (int)pad,
                                                                                   (int)math);
  Tensor ws = workspace(dy, nb);
  check_rc(xb ? (TR ? ic_conv_transpose2d_wgrad_xb : ic_conv2d_wgrad_xb)(&ax, xb->data_ptr(), &ag, dyb->data_ptr(), k,
                                                                        (int)stride, (int)pad, dw, db, (int)math,
                                                                        ws.data_ptr(), nb, stream_of(dy))
              : (TR ? ic_conv_transpose2d_wgrad_ex : ic_conv2d_wgrad_ex)(&ax, &ag, k, (int)stride, (int)pad, dw, db,
                                                                        (int)math, ws.data_ptr(), nb, stream_of(dy)),
           what);
  return out;
}

// The registered ops.  dx's memory format (the last argument of conv_dgrad): conv2d_dgrad gives dx x's own, every
// other input gradient the format of x's channel count.  The two differ only for an x of >= 32 channels that is
// not channels-last or an x of < 32 channels that is; functional passes neither (functional._cl).
Tensor conv2d_fwd(const Tensor& x, const Tensor& w, const c10::optional<Tensor>& b, int64_t stride, int64_t pad,
                  int64_t act, int64_t math) {
  return conv_fwd<false>("conv2d_fwd", x, nullptr, w, b, stride, pad, 0, act, math, nullptr);
}
Tensor conv2d_fwd_ws(const Tensor& x, const Tensor& w, const c10::optional<Tensor>& b, int64_t stride, int64_t pad,
                     int64_t act, int64_t math, Tensor& ws) {
  return conv_fwd<false>("conv2d_fwd_ws", x, nullptr, w, b, stride, pad, 0, act, math, &ws);
}
Tensor conv2d_fwd_xb(const Tensor& x, const Tensor& xb, const Tensor& w, const c10::optional<Tensor>& b, int64_t stride,
                     int64_t pad, int64_t act, int64_t math) {
  return conv_fwd<false>("conv2d_fwd_xb", x, &xb, w, b, stride, pad, 0, act, math, nullptr);
}
Tensor conv_transpose2d_fwd(const Tensor& x, const Tensor& w, const c10::optional<Tensor>& b, int64_t stride,
                            int64_t pad, int64_t opad, int64_t act, int64_t math) {
  return conv_fwd<true>("conv_transpose2d_fwd", x, nullptr, w, b, stride, pad, opad, act, math, nullptr);
}
Tensor conv_transpose2d_fwd_ws(const Tensor& x, const Tensor& w, const c10::optional<Tensor>& b, int64_t stride,
                               int64_t pad, int64_t opad, int64_t act, int64_t math, Tensor& ws) {
  return conv_fwd<true>("conv_transpose2d_fwd_ws", x, nullptr, w, b, stride, pad, opad, act, math, &ws);
}
Tensor conv_transpose2d_fwd_xb(const Tensor& x, const Tensor& xb, const Tensor& w, const c10::optional<Tensor>& b,
                               int64_t stride, int64_t pad, int64_t opad, int64_t act, int64_t math) {
  return conv_fwd<true>("conv_transpose2d_fwd_xb", x, &xb, w, b, stride, pad, opad, act, math, nullptr);
}
Tensor conv2d_dgrad(const Tensor& dy, const Tensor& w, const Tensor& x, int64_t stride, int64_t pad, int64_t math) {
  return conv_dgrad<false>("conv2d_dgrad", dy, nullptr, w, x, stride, pad, math, true);
}
Tensor conv2d_dgrad_xb(const Tensor& dy, const Tensor& dyb, const Tensor& w, const Tensor& x, int64_t stride,
                       int64_t pad, int64_t math) {
  return conv_dgrad<false>("conv2d_dgrad_xb", dy, &dyb, w, x, stride, pad, math, false);
}
Tensor conv_transpose2d_dgrad(const Tensor& dy, const Tensor& w, const Tensor& x, int64_t stride, int64_t pad,
                              int64_t math) {
  return conv_dgrad<true>("conv_transpose2d_dgrad", dy, nullptr, w, x, stride, pad, math, false);
}
Tensor conv_transpose2d_dgrad_xb(const Tensor& dy, const Tensor& dyb, const Tensor& w, const Tensor& x, int64_t stride,
                                 int64_t pad, int64_t math) {
  return conv_dgrad<true>("conv_transpose2d_dgrad_xb", dy, &dyb, w, x, stride, pad, math, false);
}
std::tuple<Tensor, Tensor> conv2d_wgrad(const Tensor& x, const Tensor& dy, const Tensor& w, int64_t stride, int64_t pad,
                                        bool bias, int64_t math) {
  return conv_wgrad<false>("conv2d_wgrad", x, nullptr, dy, nullptr, w, stride, pad, bias, math);
}
std::tuple<Tensor, Tensor> conv2d_wgrad_xb(const Tensor& x, const Tensor& xb, const Tensor& dy, const Tensor& dyb,
                                           const Tensor& w, int64_t stride, int64_t pad, bool bias, int64_t math) {
  return conv_wgrad<false>("conv2d_wgrad_xb", x, &xb, dy, &dyb, w, stride, pad, bias, math);
}
std::tuple<Tensor, Tensor> conv_transpose2d_wgrad(const Tensor& x, const Tensor& dy, const Tensor& w, int64_t stride,
                                                  int64_t pad, bool bias, int64_t math) {
  return conv_wgrad<true>("conv_transpose2d_wgrad", x, nullptr, dy, nullptr, w, stride, pad, bias, math);
}
std::tuple<Tensor, Tensor> conv_transpose2d_wgrad_xb(const Tensor& x, const Tensor& xb, const Tensor& dy,
                                                     const Tensor& dyb, const Tensor& w, int64_t stride, int64_t pad,
                                                     bool bias, int64_t math) {
  return conv_wgrad<true>("conv_transpose2d_wgrad_xb", x, &xb, dy, &dyb, w, stride, pad, bias, math);
}

// ---------------------------------------------------------------- GDN
// gamma [C][C] (or [C][C][1][1]), beta [C], already re-parameterised (NonNegativeParam).  One launcher for the
// forwards and one for the backwards; what varies (include/imgcomp.h ic_gdn_*):
//   norm: stored by the forward and read by the backward, or left out and formed again by the backward from x,
//         gamma and beta (_rn: C3, round 6), which then takes beta where the others take norm;
//   the bf16 copy of y / dx beside the fp32 tensor, of the same shape and strides (_xb, _rn: C3), for the conv that
//         reads it: no such output, an empty bf16 tensor in its place, or the copy;
//   dxsum: the column sums of dx over all pixels (the producing conv's bias gradient).
enum class Copy { None, Empty, Full };

Tensor copy_out(const Tensor& x, Copy copy) {
  if (copy == Copy::None) return Tensor();
  return copy == Copy::Full ? at::empty_like(x, x.options().dtype(at::kBFloat16))
                            : at::empty({0}, x.options().dtype(at::kBFloat16));
}

struct GdnFwd {
  Tensor y, norm, yb;
};
GdnFwd gdn_fwd_out(const Tensor& x, bool norm, Copy copy) {
  return {at::empty_like(x), norm ? at::empty_like(x) : Tensor(), copy_out(x, copy)};
}

struct GdnBwd {
  Tensor dx, dg, dbeta, dxsum, dxb;
};
GdnBwd gdn_bwd_out(const Tensor& x, const Tensor& gamma, bool sum, Copy copy) {
  return {at::empty_like(x), at::empty_like(gamma, at::MemoryFormat::Contiguous), at::empty({x.size(1)}, gamma.options()),
          sum ? at::empty({x.size(1)}, gamma.options()) : Tensor(), copy_out(x, copy)};
}

GdnFwd gdn_forward(const char* what, const Tensor& x, const Tensor& gamma, const Tensor& beta, bool inverse,
                   int64_t math, bool norm, Copy copy) {
  check_operand(x, "x");
  check_operand(gamma, "gamma");
  check_operand(beta, "beta");
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(x.device());
  TORCH_CHECK(gamma.numel() == x.size(1) * x.size(1) && beta.numel() == x.size(1), "gdn: parameters do not match ",
              x.sizes());
  GdnFwd o = gdn_fwd_out(x, norm, copy);
  const ic_act ax = act_of(x), ay = act_of(o.y);
  const size_t nb = ic_gdn_fwd_ws_ex(&ax, (int)math);
  Tensor ws = workspace(x, nb);
  const float *g = gamma.data_ptr<float>(), *b = beta.data_ptr<float>();
  void* yb = copy == Copy::Full ? o.yb.data_ptr() : nullptr;
  const int inv = inverse ? 1 : 0;
  check_rc(!norm ? ic_gdn_fwd_rn(&ax, g, b, inv, &ay, yb, (int)math, ws.data_ptr(), nb, stream_of(x))
           : copy == Copy::Full
               ? ic_gdn_fwd_xb(&ax, g, b, inv, &ay, o.norm.data_ptr<float>(), yb, (int)math, ws.data_ptr(), nb, stream_of(x))
               : ic_gdn_fwd_ex(&ax, g, b, inv, &ay, o.norm.data_ptr<float>(), (int)math, ws.data_ptr(), nb, stream_of(x)),
           what);
  return o;
}

// nob: norm, or beta when the backward forms norm again (rn).  dy must have x's strides (the caller matches them).
GdnBwd gdn_backward(const char* what, const Tensor& x, const Tensor& nob, bool rn, const Tensor& dy, const Tensor& gamma,
                    bool inverse, int64_t math, bool sum, Copy copy) {
  check_operand(x, "x");
  check_operand(dy, "dy");
  check_operand(nob, rn ? "beta" : "norm");
  check_operand(gamma, "gamma");
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(x.device());
  TORCH_CHECK(dy.sizes() == x.sizes() && dy.strides() == x.strides(), what, ": dy must have x's shape and strides");
  TORCH_CHECK(!rn || nob.numel() == x.size(1), what, ": beta does not match ", x.sizes());
  TORCH_CHECK(rn || (nob.sizes() == x.sizes() && nob.strides() == x.strides()), what,
              ": norm must have x's shape and strides");
  TORCH_CHECK(gamma.numel() == x.size(1) * x.size(1), "gdn: parameters do not match ", x.sizes());
  GdnBwd o = gdn_bwd_out(x, gamma, sum, copy);
  const ic_act ax = act_of(x), adx = act_of(o.dx);
  const size_t wb = ic_gdn_bwd_ws(&ax);
  Tensor ws = workspace(x, wb);
  const float *np = nob.data_ptr<float>(), *gy = dy.data_ptr<float>(), *g = gamma.data_ptr<float>();
  float *dg = o.dg.data_ptr<float>(), *dbeta = o.dbeta.data_ptr<float>();
  float* dxsum = sum ? o.dxsum.data_ptr<float>() : nullptr;
  void* dxb = copy == Copy::Full ? o.dxb.data_ptr() : nullptr;
  const int inv = inverse ? 1 : 0;
  check_rc(!sum ? ic_gdn_bwd_ex(&ax, np, gy, g, inv, &adx, dg, dbeta, (int)math, ws.data_ptr(), wb, stream_of(x))
           : rn ? ic_gdn_bwd_sum_rn(&ax, np, gy, g, inv, &adx, dg, dbeta, dxsum, dxb, (int)math, ws.data_ptr(), wb,
                                     stream_of(x))
           : copy == Copy::Full
               ? ic_gdn_bwd_sum_xb(&ax, np, gy, g, inv, &adx, dg, dbeta, dxsum, dxb, (int)math, ws.data_ptr(), wb,
                                   stream_of(x))
               : ic_gdn_bwd_sum_ex(&ax, np, gy, g, inv, &adx, dg, dbeta, dxsum, (int)math, ws.data_ptr(), wb,
                                   stream_of(x)),
           what);
  return o;
}

std::tuple<Tensor, Tensor> gdn_fwd(const Tensor& x, const Tensor& gamma, const Tensor& beta, bool inverse,
                                   int64_t math) {
  GdnFwd o = gdn_forward("gdn_fwd", x, gamma, beta, inverse, math, true, Copy::None);
  return {o.y, o.norm};
}
std::tuple<Tensor, Tensor, Tensor> gdn_fwd_xb(const Tensor& x, const Tensor& gamma, const Tensor& beta, bool inverse,
                                              int64_t math) {
  GdnFwd o = gdn_forward("gdn_fwd_xb", x, gamma, beta, inverse, math, true, Copy::Full);
  return {o.y, o.norm, o.yb};
}
std::tuple<Tensor, Tensor> gdn_fwd_rn(const Tensor& x, const Tensor& gamma, const Tensor& beta, bool inverse,
                                      int64_t math, bool xb) {
  GdnFwd o = gdn_forward("gdn_fwd_rn", x, gamma, beta, inverse, math, false, xb ? Copy::Full : Copy::Empty);
  return {o.y, o.yb};
}
std::tuple<Tensor, Tensor, Tensor> gdn_bwd(const Tensor& x, const Tensor& norm, const Tensor& dy, const Tensor& gamma,
                                           bool inverse, int64_t math) {
  GdnBwd o = gdn_backward("gdn_bwd", x, norm, false, dy, gamma, inverse, math, false, Copy::None);
  return {o.dx, o.dg, o.dbeta};
}
std::tuple<Tensor, Tensor, Tensor, Tensor> gdn_bwd_sum(const Tensor& x, const Tensor& norm, const Tensor& dy,
                                                       const Tensor& gamma, bool inverse, int64_t math) {
  GdnBwd o = gdn_backward("gdn_bwd_sum", x, norm, false, dy, gamma, inverse, math, true, Copy::None);
  return {o.dx, o.dg, o.dbeta, o.dxsum};
}
std::tuple<Tensor, Tensor, Tensor, Tensor, Tensor> gdn_bwd_sum_xb(const Tensor& x, const Tensor& norm, const Tensor& dy,
                                                                  const Tensor& gamma, bool inverse, int64_t math) {
  GdnBwd o = gdn_backward("gdn_bwd_sum_xb", x, norm, false, dy, gamma, inverse, math, true, Copy::Full);
  return {o.dx, o.dg, o.dbeta, o.dxsum, o.dxb};
}
std::tuple<Tensor, Tensor, Tensor, Tensor, Tensor> gdn_bwd_sum_rn(const Tensor& x, const Tensor& beta, const Tensor& dy,
                                                                  const Tensor& gamma, bool inverse, int64_t math,
                                                                  bool xb) {
  GdnBwd o = gdn_backward("gdn_bwd_sum_rn", x, beta, true, dy, gamma, inverse, math, true, xb ? Copy::Full : Copy::Empty);
  return {o.dx, o.dg, o.dbeta, o.dxsum, o.dxb};
}

// ---------------------------------------------------------------- elementwise, losses, entropy models
// Reference interfaces: NonNegativeParam.forward (layers/gdn.py:59-62), Lower/UpperBound
// (layers/bound.py:28-59), ReLU / torch.abs (prior_analysis.py:65, bmshl2018.py:72), the exp-clamp of
// prior_synthesis.py:72, _ce_loss (blocks/entropy_model.py:171-185), nn.MSELoss (loss.py:25),
// EntropyModel / CDFEstimator (entropy_model.py:47-269), SymmetricConditionalModel and its Laplacian /
// Gaussian kinds (entropy_model.py:272-378), SSIMLoss / MS_SSIMLoss (loss.py:48-188).
// The elementwise launchers index dense storage: every operand of one call has the same strides.
void check_dense(const Tensor& t, const char* what) {
  check_operand(t, what);
  TORCH_CHECK(t.is_non_overlapping_and_dense(), "imgcomp: ", what, " must be dense (non-overlapping) storage");
}

// same shape and the same strides on every dimension of extent > 1 (a size-1 dimension's
// stride addresses nothing): element i of the dense storage is the same logical element in both
bool same_layout(const Tensor& a, const Tensor& b) {
  if (a.sizes() != b.sizes()) return false;
  for (int64_t i = 0; i < a.dim(); ++i)
    if (a.size(i) > 1 && a.stride(i) != b.stride(i)) return false;
  return true;
}

void check_same_layout(const Tensor& a, const Tensor& b, const char* what) {
  check_dense(b, what);
  TORCH_CHECK(same_layout(a, b), "imgcomp: ", what, " must have the shape and strides of its partner operand");
}

Tensor like(const Tensor& t) { return at::empty_like(t, at::MemoryFormat::Preserve); }
Tensor none_like(const Tensor& t) { return at::empty({0}, t.options()); }

Tensor nonneg_fwd(const Tensor& p, double bound, double ped) {
  check_dense(p, "param");
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(p.device());
  Tensor out = like(p);
  check_rc(ic_nonneg_fwd(p.data_ptr<float>(), p.numel(), (float)bound, (float)ped, out.data_ptr<float>(), stream_of(p)),
           "nonneg_fwd");
  return out;
}
Tensor nonneg_bwd(const Tensor& p, const Tensor& g, double bound) {
  check_dense(p, "param");
  check_same_layout(p, g, "gradient");
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(p.device());
  Tensor gi = like(p);
  check_rc(ic_nonneg_bwd(p.data_ptr<float>(), g.data_ptr<float>(), p.numel(), (float)bound, gi.data_ptr<float>(),
                         stream_of(p)),
           "nonneg_bwd");
  return gi;
}
// NonNegativeParam of several tensors, one launch (ic_nonneg_multi)
std::vector<Tensor> nonneg_multi_run(at::TensorList p, at::TensorList g, at::ArrayRef<double> bound,
                                     at::ArrayRef<double> ped, bool bwd) {
  TORCH_CHECK(p.size() == bound.size() && (bwd ? g.size() == p.size() : ped.size() == p.size()),
              "nonneg_multi: one bound (and pedestal / gradient) per tensor");
  std::vector<Tensor> outs;
  std::vector<ic_nonneg_tensor> ts(p.size());
  for (size_t i = 0; i < p.size(); ++i) {
    check_dense(p[i], "param");
    TORCH_CHECK(p[i].device() == p[0].device(), "nonneg_multi: tensors on one device");
    if (bwd) check_same_layout(p[i], g[i], "gradient");
    outs.push_back(like(p[i]));
    ts[i] = ic_nonneg_tensor{p[i].data_ptr<float>(), bwd ? nullptr : outs[i].data_ptr<float>(),
                             bwd ? g[i].data_ptr<float>() : nullptr, bwd ? outs[i].data_ptr<float>() : nullptr,
                             (long long)p[i].numel(), (float)bound[i], bwd ? 0.f : (float)ped[i]};
  }
  if (p.empty()) return outs;
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(p[0].device());
  check_rc(ic_nonneg_multi(ts.data(), (int)ts.size(), bwd ? 1 : 0, stream_of(p[0])), "nonneg_multi");
  return outs;
}
std::vector<Tensor> nonneg_multi_fwd(at::TensorList p, at::ArrayRef<double> bound, at::ArrayRef<double> ped) {
  return nonneg_multi_run(p, {}, bound, ped, false);
}
std::vector<Tensor> nonneg_multi_bwd(at::TensorList p, at::TensorList g, at::ArrayRef<double> bound) {
  return nonneg_multi_run(p, g, bound, {}, true);
}
Tensor bound_fwd(const Tensor& x, double bound, bool upper) {
  check_dense(x, "x");
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(x.device());
  Tensor y = like(x);
  check_rc(ic_bound_fwd(x.data_ptr<float>(), x.numel(), (float)bound, upper ? 1 : 0, y.data_ptr<float>(), stream_of(x)),
           "bound_fwd");
  return y;
}
Tensor bound_bwd(const Tensor& x, const Tensor& g, double bound, bool upper) {
  check_dense(x, "x");
  check_same_layout(x, g, "gradient");
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(x.device());
  Tensor gx = like(x);
  check_rc(ic_bound_bwd(x.data_ptr<float>(), g.data_ptr<float>(), x.numel(), (float)bound, upper ? 1 : 0,
                        gx.data_ptr<float>(), stream_of(x)),
           "bound_bwd");
  return gx;
}
Tensor relu_fwd(const Tensor& x) {
  check_dense(x, "x");
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(x.device());
  Tensor y = like(x);
  check_rc(ic_relu_fwd(x.data_ptr<float>(), x.numel(), y.data_ptr<float>(), stream_of(x)), "relu_fwd");
  return y;
}
Tensor relu_bwd(const Tensor& y, const Tensor& g) {
  check_dense(y, "y");
  check_same_layout(y, g, "gradient");
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(y.device());
  Tensor gx = like(y);
  check_rc(ic_relu_bwd(y.data_ptr<float>(), g.data_ptr<float>(), y.numel(), gx.data_ptr<float>(), stream_of(y)),
           "relu_bwd");
  return gx;
}
Tensor abs_fwd(const Tensor& x) {
  check_dense(x, "x");
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(x.device());
  Tensor y = like(x);
  check_rc(ic_abs_fwd(x.data_ptr<float>(), x.numel(), y.data_ptr<float>(), stream_of(x)), "abs_fwd");
  return y;
}
Tensor abs_bwd(const Tensor& x, const Tensor& g) {
  check_dense(x, "x");
  check_same_layout(x, g, "gradient");
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(x.device());
  Tensor gx = like(x);
  check_rc(ic_abs_bwd(x.data_ptr<float>(), g.data_ptr<float>(), x.numel(), gx.data_ptr<float>(), stream_of(x)),
           "abs_bwd");
  return gx;
}
// (sigma, e = exp(v)); e is what the backward reads
std::tuple<Tensor, Tensor> exp_clamp_fwd(const Tensor& v, double lo, double hi) {
  check_dense(v, "v");
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(v.device());
  Tensor s = like(v), e = like(v);
  check_rc(ic_exp_clamp_fwd(v.data_ptr<float>(), v.numel(), (float)lo, (float)hi, s.data_ptr<float>(),
                            e.data_ptr<float>(), stream_of(v)),
           "exp_clamp_fwd");
  return {s, e};
}
Tensor exp_clamp_bwd(const Tensor& e, const Tensor& g, double lo, double hi) {
  check_dense(e, "e");
  check_same_layout(e, g, "gradient");
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(e.device());
  Tensor gv = like(e);
  check_rc(ic_exp_clamp_bwd(e.data_ptr<float>(), g.data_ptr<float>(), e.numel(), (float)lo, (float)hi,
                            gv.data_ptr<float>(), stream_of(e)),
           "exp_clamp_bwd");
  return gv;
}
Tensor ce_loss_fwd(const Tensor& p) {
  check_dense(p, "p");
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(p.device());
  Tensor out = at::empty({}, p.options());
  const size_t nb = ic_reduce_ws(p.numel());
  Tensor ws = workspace(p, nb);
  check_rc(ic_ce_loss_fwd(p.data_ptr<float>(), p.numel(), out.data_ptr<float>(), ws.data_ptr(), nb, stream_of(p)),
           "ce_loss_fwd");
  return out;
}
Tensor ce_loss_bwd(const Tensor& p, const Tensor& g) {
  check_dense(p, "p");
  check_operand(g, "gradient");
  TORCH_CHECK(g.numel() == 1, "ce_loss_bwd: the gradient of a scalar loss is one value");
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(p.device());
  Tensor gc = g.contiguous();
  Tensor gp = like(p);
  check_rc(ic_ce_loss_bwd(p.data_ptr<float>(), gc.data_ptr<float>(), p.numel(), gp.data_ptr<float>(), stream_of(p)),
           "ce_loss_bwd");
  return gp;
}
Tensor mse_fwd(const Tensor& a, const Tensor& b) {
  check_dense(a, "input");
  check_same_layout(a, b, "target");
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(a.device());
  Tensor out = at::empty({}, a.options());
  const size_t nb = ic_reduce_ws(a.numel());
  Tensor ws = workspace(a, nb);
  check_rc(ic_mse_fwd(a.data_ptr<float>(), b.data_ptr<float>(), a.numel(), out.data_ptr<float>(), ws.data_ptr(), nb,
                      stream_of(a)),
           "mse_fwd");
  return out;
}
// (ga, gb); a gradient that is not wanted comes back empty (0 elements)
std::tuple<Tensor, Tensor> mse_bwd(const Tensor& a, const Tensor& b, const Tensor& g, bool need_a, bool need_b) {
  check_dense(a, "input");
  check_same_layout(a, b, "target");
  check_operand(g, "gradient");
  TORCH_CHECK(g.numel() == 1, "mse_bwd: the gradient of a scalar loss is one value");
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(a.device());
  Tensor gc = g.contiguous();
  Tensor ga = need_a ? like(a) : none_like(a), gb = need_b ? like(b) : none_like(b);
  check_rc(ic_mse_bwd(a.data_ptr<float>(), b.data_ptr<float>(), gc.data_ptr<float>(), a.numel(),
                      need_a ? ga.data_ptr<float>() : nullptr, need_b ? gb.data_ptr<float>() : nullptr, stream_of(a)),
           "mse_bwd");
  return {ga, gb};
}
Tensor sqdiff_fwd(const Tensor& a, const Tensor& b) {
  check_dense(a, "input");
  check_same_layout(a, b, "target");
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(a.device());
  Tensor out = like(a);
  check_rc(ic_sqdiff_fwd(a.data_ptr<float>(), b.data_ptr<float>(), a.numel(), out.data_ptr<float>(), stream_of(a)),
           "sqdiff_fwd");
  return out;
}
std::tuple<Tensor, Tensor> sqdiff_bwd(const Tensor& a, const Tensor& b, const Tensor& g, bool need_a, bool need_b) {
  check_dense(a, "input");
  check_same_layout(a, b, "target");
  check_same_layout(a, g, "gradient");
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(a.device());
  Tensor ga = need_a ? like(a) : none_like(a), gb = need_b ? like(b) : none_like(b);
  check_rc(ic_sqdiff_bwd(a.data_ptr<float>(), b.data_ptr<float>(), g.data_ptr<float>(), a.numel(),
                         need_a ? ga.data_ptr<float>() : nullptr, need_b ? gb.data_ptr<float>() : nullptr, stream_of(a)),
           "sqdiff_bwd");
  return {ga, gb};
}

// ---- training noise: mode 3 takes the device Philox state {seed, base} (int64[2]) as `u`
const void* noise_ptr(const std::optional<Tensor>& u, int64_t mode, const Tensor& like_t) {
  if (mode == 0) {
    TORCH_CHECK(u.has_value() && u->defined(), "imgcomp: mode 0 needs the uniform draws u");
    check_same_layout(like_t, *u, "u");
    return u->data_ptr<float>();
  }
  if (mode == 3) {
    TORCH_CHECK(u.has_value() && u->defined() && u->is_cuda() && u->scalar_type() == at::kLong && u->numel() == 2 &&
                    u->is_contiguous(),
                "imgcomp: mode 3 needs the device Philox state (int64[2] {seed, base})");
    return u->data_ptr();
  }
  return nullptr;
}

// the factorized model's 11 fixed-width parameter tensors (DIMS [3, 3, 3]) in CDFEstimator order
ic_fact_params fact_params(at::TensorList prm) {
  TORCH_CHECK(prm.size() == 11, "factorized: expected the 11 CDF parameter tensors, got ", prm.size());
  for (const Tensor& t : prm) check_operand(t, "CDF parameter");
  const float* v[11];
  for (int i = 0; i < 11; ++i) {
    TORCH_CHECK(prm[i].is_contiguous(), "factorized: CDF parameters must be contiguous");
    v[i] = prm[i].data_ptr<float>();
  }
  return ic_fact_params{v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7], v[8], v[9], v[10]};
}

// z is the channels-last dense (N, ..., C) view: channel = flat index % C
std::tuple<Tensor, Tensor> factorized_fwd(const Tensor& z, int64_t C, at::TensorList prm, int64_t mode,
                                          const std::optional<Tensor>& u, int64_t seed, int64_t offset) {
  check_operand(z, "z");
  TORCH_CHECK(z.is_contiguous(), "factorized_fwd: z must be the contiguous channels-last view");
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(z.device());
  const ic_fact_params cp = fact_params(prm);
  Tensor q = like(z), p = like(z);
  check_rc(ic_factorized_fwd(z.data_ptr<float>(), z.numel(), (int)C, &cp, (int)mode, (const float*)noise_ptr(u, mode, z),
                             (unsigned long long)seed, (unsigned long long)offset, q.data_ptr<float>(),
                             p.data_ptr<float>(), stream_of(z)),
           "factorized_fwd");
  return {q, p};
}

const float* opt_grad(const std::optional<Tensor>& g, const Tensor& like_t, const char* what) {
  if (!g.has_value() || !g->defined()) return nullptr;
  check_same_layout(like_t, *g, what);
  return g->data_ptr<float>();
}

std::tuple<Tensor, std::vector<Tensor>> factorized_bwd(const Tensor& q, int64_t C, at::TensorList prm,
                                                       const std::optional<Tensor>& dq, const std::optional<Tensor>& dp) {
  check_operand(q, "q");
  TORCH_CHECK(q.is_contiguous(), "factorized_bwd: q must be contiguous");
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(q.device());
  const ic_fact_params cp = fact_params(prm);
  std::vector<Tensor> grads;
  for (const Tensor& t : prm) grads.push_back(at::empty_like(t));
  float* g[11];
  for (int i = 0; i < 11; ++i) g[i] = grads[i].data_ptr<float>();
  const ic_fact_grads cg{g[0], g[1], g[2], g[3], g[4], g[5], g[6], g[7], g[8], g[9], g[10]};
  Tensor dz = like(q);
  check_rc(ic_factorized_bwd(q.data_ptr<float>(), q.numel(), (int)C, &cp, opt_grad(dq, q, "dq"), opt_grad(dp, q, "dp"),
                             dz.data_ptr<float>(), &cg, stream_of(q)),
           "factorized_bwd");
  return {dz, grads};
}

// any CDF MLP: dims = {1, DIMS..., 1}; params [w0, b0, f0, w1, b1, f1, ..., w_last, b_last]
ic_fact_net fact_net(at::IntArrayRef dims, at::TensorList prm) {
  const int L = (int)dims.size() - 1;
  TORCH_CHECK(L >= 1 && L <= IC_FACT_NET_MAXL, "factorized: CDF MLP of ", L, " layers (at most ", IC_FACT_NET_MAXL,
              ")");
  TORCH_CHECK((int64_t)prm.size() == 3 * L - 1, "factorized: expected ", 3 * L - 1, " CDF parameter tensors");
  ic_fact_net net{};
  net.nlayers = L;
  for (int i = 0; i <= L; ++i) net.dims[i] = (int)dims[i];
  int k = 0;
  for (int l = 0; l < L; ++l) {
    for (int j = 0; j < (l < L - 1 ? 3 : 2); ++j) {
      check_operand(prm[k + j], "CDF parameter");
      TORCH_CHECK(prm[k + j].is_contiguous(), "factorized: CDF parameters must be contiguous");
    }
    net.w[l] = prm[k].data_ptr<float>();
    net.b[l] = prm[k + 1].data_ptr<float>();
    net.f[l] = l < L - 1 ? prm[k + 2].data_ptr<float>() : nullptr;
    k += l < L - 1 ? 3 : 2;
  }
  return net;
}

std::tuple<Tensor, Tensor> factorized_net_fwd(const Tensor& z, int64_t C, at::IntArrayRef dims, double bin,
                                              at::TensorList prm, int64_t mode, const std::optional<Tensor>& u,
                                              int64_t seed, int64_t offset) {
  check_operand(z, "z");
  TORCH_CHECK(z.is_contiguous(), "factorized_net_fwd: z must be the contiguous channels-last view");
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(z.device());
  const ic_fact_net net = fact_net(dims, prm);
  Tensor q = like(z), p = like(z);
  const size_t nb = ic_factorized_net_ws(z.numel(), (int)C, &net, 0);  // 0: the register kernels
  Tensor ws = workspace(z, nb);
  check_rc(ic_factorized_fwd_net_ex(z.data_ptr<float>(), z.numel(), (int)C, &net, (float)bin, (int)mode,
                                    (const float*)noise_ptr(u, mode, z), (unsigned long long)seed,
                                    (unsigned long long)offset, q.data_ptr<float>(), p.data_ptr<float>(),
                                    ws.data_ptr(), nb, stream_of(z)),
           "factorized_net_fwd");
  return {q, p};
}

std::tuple<Tensor, std::vector<Tensor>> factorized_net_bwd(const Tensor& q, int64_t C, at::IntArrayRef dims, double bin,
                                                           at::TensorList prm, const std::optional<Tensor>& dq,
                                                           const std::optional<Tensor>& dp) {
  check_operand(q, "q");
  TORCH_CHECK(q.is_contiguous(), "factorized_net_bwd: q must be contiguous");
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(q.device());
  const ic_fact_net net = fact_net(dims, prm);
  std::vector<Tensor> grads;
  for (const Tensor& t : prm) grads.push_back(at::empty_like(t));
  ic_fact_net_grads g{};
  const int L = net.nlayers;
  int k = 0;
  for (int l = 0; l < L; ++l) {
    g.w[l] = grads[k].data_ptr<float>();
    g.b[l] = grads[k + 1].data_ptr<float>();
    g.f[l] = l < L - 1 ? grads[k + 2].data_ptr<float>() : nullptr;
    k += l < L - 1 ? 3 : 2;
  }
  Tensor dz = like(q);
  const size_t nb = ic_factorized_net_ws(q.numel(), (int)C, &net, 1);
  Tensor ws = workspace(q, nb);
  check_rc(ic_factorized_bwd_net_ex(q.data_ptr<float>(), q.numel(), (int)C, &net, (float)bin, opt_grad(dq, q, "dq"),
                                    opt_grad(dp, q, "dp"), dz.data_ptr<float>(), &g, ws.data_ptr(), nb, stream_of(q)),
           "factorized_net_bwd");
  return {dz, grads};
}

Tensor quantize(const Tensor& y, int64_t mode, const std::optional<Tensor>& u, int64_t seed, int64_t offset,
                double bin) {
  check_dense(y, "y");
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(y.device());
  Tensor q = like(y);
  check_rc(ic_quantize(y.data_ptr<float>(), y.numel(), (int)mode, (const float*)noise_ptr(u, mode, y),
                       (unsigned long long)seed, (unsigned long long)offset, (float)bin, q.data_ptr<float>(),
                       stream_of(y)),
           "quantize");
  return q;
}

std::tuple<Tensor, Tensor> conditional_fwd(const Tensor& y, const Tensor& scale, const std::optional<Tensor>& mean,
                                           int64_t kind, int64_t mode, const std::optional<Tensor>& u, int64_t seed,
                                           int64_t offset, double bin) {
  check_dense(y, "y");
  check_same_layout(y, scale, "scale");
  const float* mp = opt_grad(mean, y, "mean");
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(y.device());
  Tensor q = like(y), p = like(y);
  check_rc(ic_conditional_fwd_bin(y.data_ptr<float>(), scale.data_ptr<float>(), mp, y.numel(), (int)kind, (int)mode,
                                  (const float*)noise_ptr(u, mode, y), (unsigned long long)seed,
                                  (unsigned long long)offset, (float)bin, q.data_ptr<float>(), p.data_ptr<float>(),
                                  stream_of(y)),
           "conditional_fwd");
  return {q, p};
}

// (dy, dscale, dmean); an unwanted gradient comes back empty
std::tuple<Tensor, Tensor, Tensor> conditional_bwd(const Tensor& q, const Tensor& scale,
                                                   const std::optional<Tensor>& mean, int64_t kind, double bin,
                                                   const std::optional<Tensor>& dq, const std::optional<Tensor>& dp,
                                                   bool need_y, bool need_scale, bool need_mean) {
  check_dense(q, "q");
  check_same_layout(q, scale, "scale");
  const float* mp = opt_grad(mean, q, "mean");
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(q.device());
  need_mean = need_mean && mp != nullptr;
  Tensor dy = need_y ? like(q) : none_like(q), ds = need_scale ? like(q) : none_like(q),
         dm = need_mean ? like(q) : none_like(q);
  check_rc(ic_conditional_bwd_bin(q.data_ptr<float>(), scale.data_ptr<float>(), mp, q.numel(), (int)kind, (float)bin,
                                  opt_grad(dq, q, "dq"), opt_grad(dp, q, "dp"), need_y ? dy.data_ptr<float>() : nullptr,
                                  need_scale ? ds.data_ptr<float>() : nullptr, need_mean ? dm.data_ptr<float>() : nullptr,
                                  stream_of(q)),
           "conditional_bwd");
  return {dy, ds, dm};
}

// advance the device Philox base past the n draws of the previous step (in place)
void philox_advance(const Tensor& state, int64_t n) {
  TORCH_CHECK(state.is_cuda() && state.scalar_type() == at::kLong && state.numel() == 2 && state.is_contiguous(),
              "philox_advance: expected the device state int64[2] {seed, base}");
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(state.device());
  check_rc(ic_philox_advance((unsigned long long*)state.data_ptr(), (unsigned long long)n, stream_of(state)),
           "philox_advance");
}

// ---- SSIM / MS-SSIM: (loss, state); state (written here, read by the backward) sized by ic_msssim_state_bytes
std::tuple<Tensor, Tensor> msssim_fwd(const Tensor& a_, const Tensor& b_, int64_t nlev, int64_t fs, double sigma,
                                      double max_val, bool log_scale, int64_t single, double k1, double k2, double eps,
                                      at::ArrayRef<double> weights) {
  check_operand(a_, "img1");
  check_operand(b_, "img2");
  TORCH_CHECK(a_.dim() == 4 && a_.sizes() == b_.sizes(), "msssim: two images of one 4-D shape expected");
  TORCH_CHECK((int64_t)weights.size() == nlev, "msssim: one weight per level");
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(a_.device());
  const Tensor a = a_.contiguous(), b = b_.contiguous();
  const int N = (int)a.size(0), C = (int)a.size(1), H = (int)a.size(2), W = (int)a.size(3);
  const size_t sb = ic_msssim_state_bytes(N, C, H, W, (int)nlev, (int)fs);
  TORCH_CHECK(sb > 0, "ms-ssim: image ", H, "x", W, " too small for ", nlev, " levels of a ", fs, "x", fs, " window");
  Tensor state = at::empty({(int64_t)(sb / 4)}, a.options());
  const size_t nb = ic_msssim_ws(N, C, H, W, (int)nlev, (int)fs);
  Tensor ws = workspace(a, nb);
  std::vector<float> w(weights.begin(), weights.end());
  Tensor out = (single && log_scale) ? at::empty({N}, a.options()) : at::empty({}, a.options());
  check_rc(ic_msssim_fwd(a.data_ptr<float>(), b.data_ptr<float>(), N, C, H, W, (int)nlev, (int)fs, (float)sigma,
                         (float)max_val, log_scale ? 1 : 0, (int)single, (float)k1, (float)k2, (float)eps, w.data(),
                         out.data_ptr<float>(), state.data_ptr<float>(), ws.data_ptr(), nb, stream_of(a)),
           "msssim_fwd");
  return {out, state};
}

std::tuple<Tensor, Tensor> msssim_bwd(const Tensor& g_, const Tensor& state, at::IntArrayRef shape, int64_t nlev,
                                      int64_t fs, double sigma, double max_val, bool log_scale, int64_t single,
                                      double k1, double k2, double eps, at::ArrayRef<double> weights, bool need_a,
                                      bool need_b) {
  check_operand(g_, "gradient");
  check_operand(state, "state");
  TORCH_CHECK(shape.size() == 4 && (int64_t)weights.size() == nlev, "msssim_bwd: 4-D shape and one weight per level");
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(g_.device());
  const Tensor g = g_.contiguous();
  const int N = (int)shape[0], C = (int)shape[1], H = (int)shape[2], W = (int)shape[3];
  TORCH_CHECK((size_t)state.numel() * 4 >= ic_msssim_state_bytes(N, C, H, W, (int)nlev, (int)fs),
              "msssim_bwd: state too small for this shape");
  const size_t nb = ic_msssim_ws(N, C, H, W, (int)nlev, (int)fs);
  Tensor ws = workspace(g, nb);
  std::vector<float> w(weights.begin(), weights.end());
  Tensor ga = need_a ? at::empty(shape, g.options()) : none_like(g);
  Tensor gb = need_b ? at::empty(shape, g.options()) : none_like(g);
  check_rc(ic_msssim_bwd(N, C, H, W, (int)nlev, (int)fs, (float)sigma, (float)max_val, log_scale ? 1 : 0, (int)single,
                         (float)k1, (float)k2, (float)eps, w.data(), g.data_ptr<float>(), state.data_ptr<float>(),
                         need_a ? ga.data_ptr<float>() : nullptr, need_b ? gb.data_ptr<float>() : nullptr,
                         ws.data_ptr(), nb, stream_of(g)),
           "msssim_bwd");
  return {ga, gb};
}

// ---------------------------------------------------------------- shape (Meta) kernels
// conv / GDN: the *_out function of the op's family (above), with the op's own choices
Tensor conv2d_fwd_meta(const Tensor& x, const Tensor& w, const c10::optional<Tensor>&, int64_t stride, int64_t pad,
                       int64_t, int64_t) {
  return conv_fwd_out<false>(x, w, stride, pad, 0);
}
Tensor conv2d_fwd_ws_meta(const Tensor& x, const Tensor& w, const c10::optional<Tensor>&, int64_t stride, int64_t pad,
                          int64_t, int64_t, Tensor&) {
  return conv_fwd_out<false>(x, w, stride, pad, 0);
}
Tensor conv2d_fwd_xb_meta(const Tensor& x, const Tensor&, const Tensor& w, const c10::optional<Tensor>&, int64_t stride,
                          int64_t pad, int64_t, int64_t) {
  return conv_fwd_out<false>(x, w, stride, pad, 0);
}
Tensor conv_transpose2d_fwd_meta(const Tensor& x, const Tensor& w, const c10::optional<Tensor>&, int64_t stride,
                                 int64_t pad, int64_t opad, int64_t, int64_t) {
  return conv_fwd_out<true>(x, w, stride, pad, opad);
}
Tensor conv_transpose2d_fwd_ws_meta(const Tensor& x, const Tensor& w, const c10::optional<Tensor>&, int64_t stride,
                                    int64_t pad, int64_t opad, int64_t, int64_t, Tensor&) {
  return conv_fwd_out<true>(x, w, stride, pad, opad);
}
Tensor conv_transpose2d_fwd_xb_meta(const Tensor& x, const Tensor&, const Tensor& w, const c10::optional<Tensor>&,
                                    int64_t stride, int64_t pad, int64_t opad, int64_t, int64_t) {
  return conv_fwd_out<true>(x, w, stride, pad, opad);
}
template <bool LIKE_X>  // conv2d_dgrad alone
Tensor conv_dgrad_meta(const Tensor& dy, const Tensor&, const Tensor& x, int64_t, int64_t, int64_t) {
  return conv_dgrad_out(dy, x, LIKE_X);
}
Tensor conv_dgrad_xb_meta(const Tensor& dy, const Tensor&, const Tensor&, const Tensor& x, int64_t, int64_t, int64_t) {
  return conv_dgrad_out(dy, x, false);
}
template <bool TR>
std::tuple<Tensor, Tensor> conv_wgrad_meta(const Tensor&, const Tensor&, const Tensor& w, int64_t, int64_t, bool bias,
                                           int64_t) {
  return conv_wgrad_out<TR>(w, bias);
}
template <bool TR>
std::tuple<Tensor, Tensor> conv_wgrad_xb_meta(const Tensor&, const Tensor&, const Tensor&, const Tensor&, const Tensor& w,
                                              int64_t, int64_t, bool bias, int64_t) {
  return conv_wgrad_out<TR>(w, bias);
}
std::tuple<Tensor, Tensor> gdn_fwd_meta(const Tensor& x, const Tensor&, const Tensor&, bool, int64_t) {
  GdnFwd o = gdn_fwd_out(x, true, Copy::None);
  return {o.y, o.norm};
}
std::tuple<Tensor, Tensor, Tensor> gdn_fwd_xb_meta(const Tensor& x, const Tensor&, const Tensor&, bool, int64_t) {
  GdnFwd o = gdn_fwd_out(x, true, Copy::Full);
  return {o.y, o.norm, o.yb};
}
std::tuple<Tensor, Tensor> gdn_fwd_rn_meta(const Tensor& x, const Tensor&, const Tensor&, bool, int64_t, bool xb) {
  GdnFwd o = gdn_fwd_out(x, false, xb ? Copy::Full : Copy::Empty);
  return {o.y, o.yb};
}
std::tuple<Tensor, Tensor, Tensor> gdn_bwd_meta(const Tensor& x, const Tensor&, const Tensor&, const Tensor& gamma, bool,
                                                int64_t) {
  GdnBwd o = gdn_bwd_out(x, gamma, false, Copy::None);
  return {o.dx, o.dg, o.dbeta};
}
std::tuple<Tensor, Tensor, Tensor, Tensor> gdn_bwd_sum_meta(const Tensor& x, const Tensor&, const Tensor&,
                                                            const Tensor& gamma, bool, int64_t) {
  GdnBwd o = gdn_bwd_out(x, gamma, true, Copy::None);
  return {o.dx, o.dg, o.dbeta, o.dxsum};
}
std::tuple<Tensor, Tensor, Tensor, Tensor, Tensor> gdn_bwd_sum_xb_meta(const Tensor& x, const Tensor&, const Tensor&,
                                                                       const Tensor& gamma, bool, int64_t) {
  GdnBwd o = gdn_bwd_out(x, gamma, true, Copy::Full);
  return {o.dx, o.dg, o.dbeta, o.dxsum, o.dxb};
}
std::tuple<Tensor, Tensor, Tensor, Tensor, Tensor> gdn_bwd_sum_rn_meta(const Tensor& x, const Tensor&, const Tensor&,
                                                                       const Tensor& gamma, bool, int64_t, bool xb) {
  GdnBwd o = gdn_bwd_out(x, gamma, true, xb ? Copy::Full : Copy::Empty);
  return {o.dx, o.dg, o.dbeta, o.dxsum, o.dxb};
}

// elementwise / loss / entropy shape kernels
Tensor like_meta1(const Tensor& x) { return at::empty_like(x, at::MemoryFormat::Preserve); }
Tensor nonneg_fwd_meta(const Tensor& p, double, double) { return like_meta1(p); }
Tensor nonneg_bwd_meta(const Tensor& p, const Tensor&, double) { return like_meta1(p); }
std::vector<Tensor> nonneg_multi_fwd_meta(at::TensorList p, at::ArrayRef<double>, at::ArrayRef<double>) {
  std::vector<Tensor> o;
  for (const auto& t : p) o.push_back(like_meta1(t));
  return o;
}
std::vector<Tensor> nonneg_multi_bwd_meta(at::TensorList p, at::TensorList, at::ArrayRef<double>) {
  std::vector<Tensor> o;
  for (const auto& t : p) o.push_back(like_meta1(t));
  return o;
}
Tensor bound_fwd_meta(const Tensor& x, double, bool) { return like_meta1(x); }
Tensor bound_bwd_meta(const Tensor& x, const Tensor&, double, bool) { return like_meta1(x); }
Tensor unary_meta(const Tensor& x) { return like_meta1(x); }
Tensor binary_meta(const Tensor& x, const Tensor&) { return like_meta1(x); }
std::tuple<Tensor, Tensor> exp_clamp_fwd_meta(const Tensor& v, double, double) { return {like_meta1(v), like_meta1(v)}; }
Tensor exp_clamp_bwd_meta(const Tensor& e, const Tensor&, double, double) { return like_meta1(e); }
Tensor scalar_loss_meta1(const Tensor& p) { return at::empty({}, p.options()); }
Tensor scalar_loss_meta2(const Tensor& a, const Tensor&) { return at::empty({}, a.options()); }
Tensor ce_loss_bwd_meta(const Tensor& p, const Tensor&) { return like_meta1(p); }
std::tuple<Tensor, Tensor> pair_grad_meta(const Tensor& a, const Tensor& b, const Tensor&, bool need_a, bool need_b) {
  return {need_a ? like_meta1(a) : at::empty({0}, a.options()), need_b ? like_meta1(b) : at::empty({0}, b.options())};
}
std::tuple<Tensor, Tensor> factorized_fwd_meta(const Tensor& z, int64_t, at::TensorList, int64_t,
                                               const std::optional<Tensor>&, int64_t, int64_t) {
  return {like_meta1(z), like_meta1(z)};
}
std::tuple<Tensor, std::vector<Tensor>> factorized_bwd_meta(const Tensor& q, int64_t, at::TensorList prm,
                                                            const std::optional<Tensor>&, const std::optional<Tensor>&) {
  std::vector<Tensor> g;
  for (const Tensor& t : prm) g.push_back(at::empty_like(t));
  return {like_meta1(q), g};
}
std::tuple<Tensor, Tensor> factorized_net_fwd_meta(const Tensor& z, int64_t, at::IntArrayRef, double, at::TensorList,
                                                   int64_t, const std::optional<Tensor>&, int64_t, int64_t) {
  return {like_meta1(z), like_meta1(z)};
}
std::tuple<Tensor, std::vector<Tensor>> factorized_net_bwd_meta(const Tensor& q, int64_t, at::IntArrayRef, double,
                                                                at::TensorList prm, const std::optional<Tensor>&,
                                                                const std::optional<Tensor>&) {
  std::vector<Tensor> g;
  for (const Tensor& t : prm) g.push_back(at::empty_like(t));
  return {like_meta1(q), g};
}
Tensor quantize_meta(const Tensor& y, int64_t, const std::optional<Tensor>&, int64_t, int64_t, double) {
  return like_meta1(y);
}
std::tuple<Tensor, Tensor> conditional_fwd_meta(const Tensor& y, const Tensor&, const std::optional<Tensor>&, int64_t,
                                                int64_t, const std::optional<Tensor>&, int64_t, int64_t, double) {
  return {like_meta1(y), like_meta1(y)};
}
std::tuple<Tensor, Tensor, Tensor> conditional_bwd_meta(const Tensor& q, const Tensor&, const std::optional<Tensor>& mean,
                                                        int64_t, double, const std::optional<Tensor>&,
                                                        const std::optional<Tensor>&, bool need_y, bool need_scale,
                                                        bool need_mean) {
  const Tensor e = at::empty({0}, q.options());
  need_mean = need_mean && mean.has_value() && mean->defined();
  return {need_y ? like_meta1(q) : e, need_scale ? like_meta1(q) : e, need_mean ? like_meta1(q) : e};
}
void philox_advance_meta(const Tensor&, int64_t) {}
std::tuple<Tensor, Tensor> msssim_fwd_meta(const Tensor& a, const Tensor&, int64_t nlev, int64_t fs, double, double,
                                           bool log_scale, int64_t single, double, double, double, at::ArrayRef<double>) {
  const size_t sb = ic_msssim_state_bytes((int)a.size(0), (int)a.size(1), (int)a.size(2), (int)a.size(3), (int)nlev,
                                          (int)fs);
  TORCH_CHECK(sb > 0, "ms-ssim: image too small for the levels and window");
  return {(single && log_scale) ? at::empty({a.size(0)}, a.options()) : at::empty({}, a.options()),
          at::empty({(int64_t)(sb / 4)}, a.options())};
}
std::tuple<Tensor, Tensor> msssim_bwd_meta(const Tensor& g, const Tensor&, at::IntArrayRef shape, int64_t, int64_t,
                                           double, double, bool, int64_t, double, double, double, at::ArrayRef<double>,
                                           bool need_a, bool need_b) {
  return {need_a ? at::empty(shape, g.options()) : at::empty({0}, g.options()),
          need_b ? at::empty(shape, g.options()) : at::empty({0}, g.options())};
}

// ---------------------------------------------------------------- entropy coder (imgcomp_codec)
// compress / decompress only (never the training step): symbols int32, table rows uint8, tables int32
// [rows][2K+2] (the C ABI's uint32 counts, all <= 65536), byte buffers uint8.
void check_codec(const Tensor& t, at::ScalarType ty, const char* what) {
  TORCH_CHECK(t.is_cuda(), "imgcomp_codec: ", what, " must be on a ROCm device, got ", t.device());
  TORCH_CHECK(t.scalar_type() == ty && t.is_contiguous(), "imgcomp_codec: ", what, " must be contiguous ", ty);
}

int64_t codec_k(const Tensor& cdf) {
  TORCH_CHECK(cdf.dim() == 2 && cdf.size(1) >= 2 && cdf.size(1) % 2 == 0 && cdf.size(1) <= 2 * IC_CODEC_KMAX + 2,
              "imgcomp_codec: tables must be [rows][2K+2] with K <= ", IC_CODEC_KMAX, ", got ", cdf.sizes());
  return cdf.size(1) / 2 - 1;
}

const unsigned char* codec_rows(const std::optional<Tensor>& rows, int64_t n) {
  if (!rows.has_value() || !rows->defined()) return nullptr;
  check_codec(*rows, at::kByte, "rows");
  TORCH_CHECK(rows->numel() == n, "imgcomp_codec: one table row per symbol");
  return rows->data_ptr<unsigned char>();
}

// The four symbolizers (symbolize / symbolize_seg here, of imgcomp_stream and of imgcomp_mean): x, about mu where
// given, to its symbols, as one run (seg false, nseg 1) or as nseg equal segments.  Returns sym and each
// segment's largest magnitude; one over the coder's limit is a ValueError under the op's namespace `ns`.
Tensor symbols_out(const Tensor& x) { return at::empty({x.numel()}, x.options().dtype(at::kInt)); }

std::tuple<Tensor, std::vector<int64_t>> symbolize(const char* ns, const char* what, const Tensor& x, const Tensor* mu,
                                                   bool seg, int64_t nseg) {
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(x.device());
  Tensor sym = symbols_out(x);
  Tensor kd = at::empty({nseg}, x.options().dtype(at::kInt));
  std::vector<int> kmax((size_t)nseg, 0);
  const float* xp = x.data_ptr<float>();
  const float* mp = mu ? mu->data_ptr<float>() : nullptr;
  const int64_t n = x.numel();
  int *sp = sym.data_ptr<int>(), *kp = kd.data_ptr<int>();
  const int rc = seg ? (mu ? ic_codec_symbolize_mean_seg(xp, mp, (int)nseg, n / nseg, sp, kp, kmax.data(), stream_of(x))
                           : ic_codec_symbolize_seg(xp, (int)nseg, n / nseg, sp, kp, kmax.data(), stream_of(x)))
                     : (mu ? ic_codec_symbolize_mean(xp, mp, n, sp, kp, kmax.data(), stream_of(x))
                           : ic_codec_symbolize(xp, n, sp, kp, kmax.data(), stream_of(x)));
  if (rc == IC_ERR_ARG)
    for (int64_t s = 0; s < nseg; ++s) {
      TORCH_CHECK_VALUE(seg || kmax[s] <= IC_CODEC_KMAX, ns, ": a symbol of magnitude ", kmax[s],
                        " exceeds the coder's limit of ", IC_CODEC_KMAX);
      TORCH_CHECK_VALUE(kmax[s] <= IC_CODEC_KMAX, ns, ": image ", s, " has a symbol of magnitude ", kmax[s],
                        ", which exceeds the coder's limit of ", IC_CODEC_KMAX);
    }
  check_rc(rc, what);
  return {sym, std::vector<int64_t>(kmax.begin(), kmax.end())};
}

// The shared tail of the symbolizers that take a list of candidates (gain_symbolize_seg, requant_seg,
// block_gain_symbolize_seg): img names, for every `item` ("candidate", "target"), one of the N `source`s ("image",
// "source") of y; mu holds the items' means back to back and gives the symbols their size.  call(img, img_dev, sym,
// kmax_dev, kmax_host) makes the C call; an item over the coder's limit is a ValueError under the namespace `ns`.
template <class Call>
std::tuple<Tensor, std::vector<int64_t>> symbolize_candidates(const char* ns, const char* what, const char* item,
                                                              const char* source, const Tensor& y, const Tensor& mu,
                                                              at::IntArrayRef img, Call call) {
  const int64_t M = (int64_t)img.size(), N = y.size(0);
  std::vector<int> im;
  for (int64_t m = 0; m < M; ++m) {
    TORCH_CHECK_VALUE(img[m] >= 0 && img[m] < N, ns, ": ", item, " ", m, " names ", source, " ", img[m], " of ", N);
    im.push_back((int)img[m]);
  }
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(y.device());
  Tensor sym = symbols_out(mu);
  Tensor kd = at::empty({2 * M}, y.options().dtype(at::kInt));   // the maxima, then img on the device
  std::vector<int> kmax((size_t)M, 0);
  const int rc = call(im.data(), kd.data_ptr<int>() + M, sym.data_ptr<int>(), kd.data_ptr<int>(), kmax.data());
  if (rc == IC_ERR_ARG)
    for (int64_t m = 0; m < M; ++m)
      TORCH_CHECK_VALUE(kmax[m] <= IC_CODEC_KMAX, ns, ": ", item, " ", m, " (", source, " ", img[m],
                        ") has a symbol of magnitude ", kmax[m], ", which exceeds the coder's limit of ", IC_CODEC_KMAX);
  check_rc(rc, what);
  return {sym, std::vector<int64_t>(kmax.begin(), kmax.end())};
}

std::tuple<Tensor, int64_t> codec_symbolize(const Tensor& x) {
  check_dense(x, "x");
  TORCH_CHECK(x.numel() > 0, "imgcomp_codec: empty tensor");
  auto r = symbolize("imgcomp_codec", "codec_symbolize", x, nullptr, false, 1);
  return {std::get<0>(r), std::get<1>(r)[0]};
}

Tensor codec_scale_index(const Tensor& sigma, at::ArrayRef<double> mids) {
  check_dense(sigma, "sigma");
  TORCH_CHECK(sigma.numel() > 0 && (int64_t)mids.size() < IC_CODEC_MAXL, "imgcomp_codec: at most ", IC_CODEC_MAXL,
              " scales");
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(sigma.device());
  std::vector<float> m(mids.begin(), mids.end());
  Tensor rows = at::empty({sigma.numel()}, sigma.options().dtype(at::kByte));
  check_rc(ic_codec_scale_index(sigma.data_ptr<float>(), sigma.numel(), m.data(), (int)m.size() + 1,
                                rows.data_ptr<unsigned char>(), stream_of(sigma)),
           "codec_scale_index");
  return rows;
}

Tensor codec_build_tables(const Tensor& pmf) {
  check_operand(pmf, "pmf");
  TORCH_CHECK(pmf.dim() == 2 && pmf.is_contiguous() && pmf.size(0) >= 1 && pmf.size(1) % 2 == 1 &&
                  pmf.size(1) <= 2 * IC_CODEC_KMAX + 1,
              "imgcomp_codec: pmf must be contiguous [rows][2K+1] with K <= ", IC_CODEC_KMAX, ", got ", pmf.sizes());
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(pmf.device());
  Tensor cdf = at::empty({pmf.size(0), pmf.size(1) + 1}, pmf.options().dtype(at::kInt));
  check_rc(ic_codec_build_tables(pmf.data_ptr<float>(), (int)pmf.size(0), (int)(pmf.size(1) / 2),
                                 (unsigned int*)cdf.data_ptr<int>(), stream_of(pmf)),
           "codec_build_tables");
  return cdf;
}

// [lengths: chunks x u32][payload], padded to the worst case (the lengths say how much is payload)
Tensor codec_encode(const Tensor& sym, const std::optional<Tensor>& rows, int64_t C, const Tensor& cdf, int64_t steps) {
  check_codec(sym, at::kInt, "sym");
  check_codec(cdf, at::kInt, "tables");
  const int64_t K = codec_k(cdf), n = sym.numel();
  const unsigned char* rp = codec_rows(rows, n);
  TORCH_CHECK(steps >= 1 && steps <= IC_CODEC_MAXR && n > 0, "imgcomp_codec: steps_per_chunk in [1, ", IC_CODEC_MAXR, "]");
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(sym.device());
  const size_t nb = ic_codec_encode_ws(n, (int)steps), ob = ic_codec_compact_bytes(n, (int)steps);
  Tensor ws = at::empty({(int64_t)nb}, sym.options().dtype(at::kByte));
  Tensor lens = at::empty({(int64_t)ic_codec_chunks(n, (int)steps)}, sym.options().dtype(at::kInt));
  Tensor out = at::empty({(int64_t)ob}, sym.options().dtype(at::kByte));
  check_rc(ic_codec_encode(sym.data_ptr<int>(), n, rp, (int)C, (const unsigned int*)cdf.data_ptr<int>(),
                           (int)cdf.size(0), (int)K, (int)steps, ws.data_ptr(), nb, (unsigned int*)lens.data_ptr<int>(),
                           stream_of(sym)),
           "codec_encode");
  check_rc(ic_codec_compact(ws.data_ptr(), (const unsigned int*)lens.data_ptr<int>(), n, (int)steps, out.data_ptr(), ob,
                            stream_of(sym)),
           "codec_compact");
  return out;
}

Tensor codec_decode(const Tensor& packed, int64_t n, const std::optional<Tensor>& rows, int64_t C, const Tensor& cdf,
                    int64_t steps) {
  check_codec(packed, at::kByte, "packed");
  check_codec(cdf, at::kInt, "tables");
  const int64_t K = codec_k(cdf);
  TORCH_CHECK(n > 0, "imgcomp_codec: no symbols");
  const unsigned char* rp = codec_rows(rows, n);
  TORCH_CHECK(steps >= 1 && steps <= IC_CODEC_MAXR, "imgcomp_codec: steps_per_chunk in [1, ", IC_CODEC_MAXR, "]");
  TORCH_CHECK(((uintptr_t)packed.data_ptr() & 3) == 0, "imgcomp_codec: packed buffer must be 4-byte aligned");
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(packed.device());
  Tensor out = at::empty({n}, packed.options().dtype(at::kFloat));
  check_rc(ic_codec_decode(packed.data_ptr(), (size_t)packed.numel(), n, rp, (int)C,
                           (const unsigned int*)cdf.data_ptr<int>(), (int)cdf.size(0), (int)K, (int)steps,
                           out.data_ptr<float>(), stream_of(packed)),
           "codec_decode");
  return out;
}

std::tuple<Tensor, int64_t> codec_symbolize_meta(const Tensor& x) { return {symbols_out(x), 0}; }
Tensor codec_scale_index_meta(const Tensor& sigma, at::ArrayRef<double>) {
  return at::empty({sigma.numel()}, sigma.options().dtype(at::kByte));
}
Tensor codec_build_tables_meta(const Tensor& pmf) {
  TORCH_CHECK(pmf.dim() == 2, "imgcomp_codec: pmf must be [rows][2K+1]");
  return at::empty({pmf.size(0), pmf.size(1) + 1}, pmf.options().dtype(at::kInt));
}
Tensor codec_encode_meta(const Tensor& sym, const std::optional<Tensor>&, int64_t, const Tensor&, int64_t steps) {
  const size_t ob = ic_codec_compact_bytes(sym.numel(), (int)steps);
  TORCH_CHECK(ob > 0, "imgcomp_codec: bad symbol count or steps_per_chunk");
  return at::empty({(int64_t)ob}, sym.options().dtype(at::kByte));
}
Tensor codec_decode_meta(const Tensor& packed, int64_t n, const std::optional<Tensor>&, int64_t, const Tensor&, int64_t) {
  return at::empty({n}, packed.options().dtype(at::kFloat));
}

// ---------------------------------------------------------------- per-image streams (imgcomp_stream)
// The segmented coder: nseg images' symbols back to back, K and table (word offset into `pool`) per image.
struct SegTables {
  std::vector<int> k;
  std::vector<long long> off;
};

SegTables seg_tables(int64_t nseg, at::IntArrayRef seg_k, at::IntArrayRef seg_off) {
  TORCH_CHECK(nseg >= 1 && nseg <= 65535 && (int64_t)seg_k.size() == nseg && (int64_t)seg_off.size() == nseg,
              "imgcomp_stream: one K and one table offset per segment");
  SegTables t;
  for (int64_t s = 0; s < nseg; ++s) {
    TORCH_CHECK(seg_k[s] >= 0 && seg_k[s] <= IC_CODEC_KMAX, "imgcomp_stream: K of segment ", s, " is ", seg_k[s],
                ", the coder's limit is ", IC_CODEC_KMAX);
    t.k.push_back((int)seg_k[s]);
    t.off.push_back(seg_off[s]);
  }
  return t;
}

std::tuple<Tensor, std::vector<int64_t>> stream_symbolize_seg(const Tensor& x, int64_t nseg) {
  check_dense(x, "x");
  TORCH_CHECK(nseg >= 1 && nseg <= 65535 && x.numel() > 0 && x.numel() % nseg == 0,
              "imgcomp_stream: ", x.numel(), " values do not make ", nseg, " equal segments");
  return symbolize("imgcomp_stream", "codec_symbolize_seg", x, nullptr, true, nseg);
}

// [lengths: all chunks x u32][payload], (segment, chunk) order, padded to the worst case
Tensor stream_encode_seg(const Tensor& sym, int64_t nseg, const std::optional<Tensor>& rows, int64_t C, const Tensor& pool,
                         int64_t nrows, at::IntArrayRef seg_k, at::IntArrayRef seg_off, int64_t steps) {
  check_codec(sym, at::kInt, "sym");
  check_codec(pool, at::kInt, "table pool");
  const SegTables t = seg_tables(nseg, seg_k, seg_off);
  const int64_t n = sym.numel();
  TORCH_CHECK(n > 0 && n % nseg == 0, "imgcomp_stream: ", n, " symbols do not make ", nseg, " equal segments");
  const unsigned char* rp = codec_rows(rows, n);
  TORCH_CHECK(steps >= 1 && steps <= IC_CODEC_MAXR, "imgcomp_stream: steps_per_chunk in [1, ", IC_CODEC_MAXR, "]");
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(sym.device());
  const int64_t seg_len = n / nseg, chunks = ic_codec_seg_chunks((int)nseg, seg_len, (int)steps);
  TORCH_CHECK(chunks > 0, "imgcomp_stream: too many chunks");
  const size_t nb = ic_codec_encode_seg_ws((int)nseg, seg_len, (int)steps);
  const size_t ob = ic_codec_compact_seg_bytes((int)nseg, seg_len, (int)steps);
  Tensor ws = at::empty({(int64_t)nb}, sym.options().dtype(at::kByte));
  Tensor lens = at::empty({chunks}, sym.options());
  Tensor kt = at::empty({2 * nseg}, sym.options());
  Tensor out = at::empty({(int64_t)ob}, sym.options().dtype(at::kByte));
  check_rc(ic_codec_encode_seg(sym.data_ptr<int>(), (int)nseg, seg_len, rp, (int)C,
                               (const unsigned int*)pool.data_ptr<int>(), (size_t)pool.numel(), (int)nrows, t.k.data(),
                               t.off.data(), kt.data_ptr<int>(), (int)steps, ws.data_ptr(), nb,
                               (unsigned int*)lens.data_ptr<int>(), stream_of(sym)),
           "codec_encode_seg");
  check_rc(ic_codec_compact_seg(ws.data_ptr(), (const unsigned int*)lens.data_ptr<int>(), chunks, (int)steps,
                                out.data_ptr(), ob, stream_of(sym)),
           "codec_compact_seg");
  return out;
}

Tensor stream_decode_seg(const Tensor& packed, int64_t nseg, int64_t seg_len, const std::optional<Tensor>& rows, int64_t C,
                         const Tensor& pool, int64_t nrows, at::IntArrayRef seg_k, at::IntArrayRef seg_off,
                         int64_t steps) {
  check_codec(packed, at::kByte, "packed");
  check_codec(pool, at::kInt, "table pool");
  const SegTables t = seg_tables(nseg, seg_k, seg_off);
  TORCH_CHECK(seg_len > 0 && seg_len <= INT64_MAX / nseg, "imgcomp_stream: no symbols");
  const unsigned char* rp = codec_rows(rows, nseg * seg_len);
  TORCH_CHECK(steps >= 1 && steps <= IC_CODEC_MAXR, "imgcomp_stream: steps_per_chunk in [1, ", IC_CODEC_MAXR, "]");
  TORCH_CHECK(((uintptr_t)packed.data_ptr() & 3) == 0, "imgcomp_stream: packed buffer must be 4-byte aligned");
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(packed.device());
  Tensor out = at::empty({nseg * seg_len}, packed.options().dtype(at::kFloat));
  Tensor kt = at::empty({2 * nseg}, packed.options().dtype(at::kInt));
  check_rc(ic_codec_decode_seg(packed.data_ptr(), (size_t)packed.numel(), (int)nseg, seg_len, rp, (int)C,
                               (const unsigned int*)pool.data_ptr<int>(), (size_t)pool.numel(), (int)nrows, t.k.data(),
                               t.off.data(), kt.data_ptr<int>(), (int)steps, out.data_ptr<float>(), stream_of(packed)),
           "codec_decode_seg");
  return out;
}

Tensor stream_pad_edge(const Tensor& x, int64_t Hp, int64_t Wp) {
  check_operand(x, "x");
  TORCH_CHECK(x.dim() == 4 && x.is_contiguous() && x.numel() > 0 && Hp >= x.size(2) && Wp >= x.size(3),
              "imgcomp_stream: pad_edge takes a contiguous (N, C, h, w) tensor and a padded size >= (h, w), got ",
              x.sizes(), " -> ", Hp, " x ", Wp);
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(x.device());
  Tensor y = at::empty({x.size(0), x.size(1), Hp, Wp}, x.options());
  check_rc(ic_pad_edge(x.data_ptr<float>(), (int)x.size(0), (int)x.size(1), (int)x.size(2), (int)x.size(3), (int)Hp,
                       (int)Wp, y.data_ptr<float>(), stream_of(x)),
           "pad_edge");
  return y;
}

Tensor stream_crop_clamp(const Tensor& x, int64_t h, int64_t w) {
  check_operand(x, "x");
  TORCH_CHECK(x.dim() == 4 && x.numel() > 0 && h >= 1 && w >= 1 && h <= x.size(2) && w <= x.size(3),
              "imgcomp_stream: crop_clamp takes (N, C, H, W) and a crop 1 <= (h, w) <= (H, W), got ", x.sizes(), " -> ",
              h, " x ", w);
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(x.device());
  Tensor y = at::empty({x.size(0), x.size(1), h, w}, x.options().memory_format(at::MemoryFormat::Contiguous));
  const ic_act ax = act_of(x);
  check_rc(ic_crop_clamp(&ax, (int)h, (int)w, y.data_ptr<float>(), stream_of(x)), "crop_clamp");
  return y;
}

std::tuple<Tensor, std::vector<int64_t>> stream_symbolize_seg_meta(const Tensor& x, int64_t nseg) {
  return {symbols_out(x), std::vector<int64_t>((size_t)std::max<int64_t>(nseg, 0), 0)};
}
Tensor stream_encode_seg_meta(const Tensor& sym, int64_t nseg, const std::optional<Tensor>&, int64_t, const Tensor&, int64_t,
                              at::IntArrayRef, at::IntArrayRef, int64_t steps) {
  TORCH_CHECK(nseg >= 1 && sym.numel() % nseg == 0, "imgcomp_stream: symbols do not make equal segments");
  const size_t ob = ic_codec_compact_seg_bytes((int)nseg, sym.numel() / nseg, (int)steps);
  TORCH_CHECK(ob > 0, "imgcomp_stream: bad symbol count or steps_per_chunk");
  return at::empty({(int64_t)ob}, sym.options().dtype(at::kByte));
}
Tensor stream_decode_seg_meta(const Tensor& packed, int64_t nseg, int64_t seg_len, const std::optional<Tensor>&, int64_t,
                              const Tensor&, int64_t, at::IntArrayRef, at::IntArrayRef, int64_t) {
  return at::empty({nseg * seg_len}, packed.options().dtype(at::kFloat));
}
Tensor stream_pad_edge_meta(const Tensor& x, int64_t Hp, int64_t Wp) {
  TORCH_CHECK(x.dim() == 4, "imgcomp_stream: pad_edge takes (N, C, h, w)");
  return at::empty({x.size(0), x.size(1), Hp, Wp}, x.options());
}
Tensor stream_crop_clamp_meta(const Tensor& x, int64_t h, int64_t w) {
  TORCH_CHECK(x.dim() == 4, "imgcomp_stream: crop_clamp takes (N, C, H, W)");
  return at::empty({x.size(0), x.size(1), h, w}, x.options().memory_format(at::MemoryFormat::Contiguous));
}

// ---------------------------------------------------------------- mean-scale hyperprior (imgcomp_mean)
// y is coded about a mean: both operands are contiguous (the channels-last storage the coder flattens), of the
// same element count in the same order; the outputs are flat, like the symbolizers' above.
void check_mean_pair(const Tensor& a, const Tensor& mu, const char* what) {
  check_operand(a, what);
  check_operand(mu, "mu");
  TORCH_CHECK(a.is_contiguous() && mu.is_contiguous(), "imgcomp_mean: ", what, " and mu must be contiguous");
  TORCH_CHECK(a.numel() > 0 && a.numel() == mu.numel() && a.device() == mu.device(), "imgcomp_mean: ", what, " (",
              a.numel(), " values) and mu (", mu.numel(), ") must hold the same number of values on one device");
}

std::tuple<Tensor, int64_t> mean_symbolize(const Tensor& y, const Tensor& mu) {
  check_mean_pair(y, mu, "y");
  auto r = symbolize("imgcomp_mean", "codec_symbolize_mean", y, &mu, false, 1);
  return {std::get<0>(r), std::get<1>(r)[0]};
}

std::tuple<Tensor, std::vector<int64_t>> mean_symbolize_seg(const Tensor& y, const Tensor& mu, int64_t nseg) {
  check_mean_pair(y, mu, "y");
  TORCH_CHECK(nseg >= 1 && nseg <= 65535 && y.numel() % nseg == 0, "imgcomp_mean: ", y.numel(), " values do not make ",
              nseg, " equal segments");
  return symbolize("imgcomp_mean", "codec_symbolize_mean_seg", y, &mu, true, nseg);
}

std::tuple<Tensor, Tensor> mean_center_round(const Tensor& y, const Tensor& mu) {
  check_mean_pair(y, mu, "y");
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(y.device());
  Tensor r = at::empty({y.numel()}, y.options());
  Tensor y_hat = at::empty({y.numel()}, y.options());
  check_rc(ic_center_round(y.data_ptr<float>(), mu.data_ptr<float>(), y.numel(), r.data_ptr<float>(),
                           y_hat.data_ptr<float>(), stream_of(y)),
           "center_round");
  return {r, y_hat};
}

Tensor mean_add(const Tensor& r, const Tensor& mu) {
  check_mean_pair(r, mu, "r");
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(r.device());
  Tensor y_hat = at::empty({r.numel()}, r.options());
  check_rc(ic_add_mean(r.data_ptr<float>(), mu.data_ptr<float>(), r.numel(), y_hat.data_ptr<float>(), stream_of(r)),
           "add_mean");
  return y_hat;
}

std::tuple<Tensor, int64_t> mean_symbolize_meta(const Tensor& y, const Tensor& mu) {
  TORCH_CHECK(y.numel() == mu.numel(), "imgcomp_mean: y and mu must hold the same number of values");
  return {symbols_out(y), 0};
}
std::tuple<Tensor, std::vector<int64_t>> mean_symbolize_seg_meta(const Tensor& y, const Tensor& mu, int64_t nseg) {
  TORCH_CHECK(y.numel() == mu.numel(), "imgcomp_mean: y and mu must hold the same number of values");
  return stream_symbolize_seg_meta(y, nseg);
}
std::tuple<Tensor, Tensor> mean_center_round_meta(const Tensor& y, const Tensor& mu) {
  TORCH_CHECK(y.numel() == mu.numel(), "imgcomp_mean: y and mu must hold the same number of values");
  return {at::empty({y.numel()}, y.options()), at::empty({y.numel()}, y.options())};
}
Tensor mean_add_meta(const Tensor& r, const Tensor& mu) {
  TORCH_CHECK(r.numel() == mu.numel(), "imgcomp_mean: r and mu must hold the same number of values");
  return at::empty({r.numel()}, r.options());
}

// ---------------------------------------------------------------- checkerboard context model (imgcomp_ckbd)
// Every full tensor is 4-D (N, H, W, C) and contiguous: the channels-last storage of a latent, position (i, j) an
// anchor when i + j is even.  A half is flat: the elements at the positions of one parity in (n, i, j, c) order.
void check_ckbd_shape(const Tensor& t, const char* what) {
  TORCH_CHECK(t.dim() == 4 && t.is_contiguous() && t.numel() > 0, "imgcomp_ckbd: ", what,
              " must be a non-empty contiguous (N, H, W, C) tensor, got ", t.sizes());
  for (int64_t d = 0; d < 4; ++d) TORCH_CHECK(t.size(d) <= INT_MAX, "imgcomp_ckbd: ", what, " is too large: ", t.sizes());
}

void check_ckbd(const Tensor& t, const char* what) {
  check_operand(t, what);
  check_ckbd_shape(t, what);
}

void check_ckbd_like(const Tensor& a, const Tensor& t, const char* what) {
  check_ckbd(t, what);
  TORCH_CHECK(t.sizes() == a.sizes() && t.device() == a.device(), "imgcomp_ckbd: ", what, " ", t.sizes(),
              " must have the shape ", a.sizes(), " of its partner operand, on one device");
}

void check_parity(int64_t parity) { TORCH_CHECK(parity == 0 || parity == 1, "imgcomp_ckbd: parity ", parity, " is not 0 or 1"); }

int64_t ckbd_half_numel(const Tensor& full, int64_t parity) {
  return full.size(0) * ic_ckbd_count((int)full.size(1), (int)full.size(2), (int)parity) * full.size(3);
}

#define CKBD_DIMS(t) (int)(t).size(0), (int)(t).size(1), (int)(t).size(2), (int)(t).size(3)

std::tuple<Tensor, Tensor> ckbd_input_fwd(const Tensor& y, const Tensor& mu) {
  check_ckbd(y, "y");
  check_ckbd_like(y, mu, "mu");
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(y.device());
  Tensor u = at::empty_like(y), v = at::empty_like(y);
  check_rc(ic_ckbd_input_fwd(y.data_ptr<float>(), mu.data_ptr<float>(), CKBD_DIMS(y), u.data_ptr<float>(),
                             v.data_ptr<float>(), stream_of(y)),
           "ckbd_input_fwd");
  return {u, v};
}

std::tuple<Tensor, Tensor> ckbd_input_bwd(const Tensor& y, const Tensor& mu, const Tensor& du, const Tensor& dv) {
  check_ckbd(y, "y");
  check_ckbd_like(y, mu, "mu");
  check_ckbd_like(y, du, "du");
  check_ckbd_like(y, dv, "dv");
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(y.device());
  Tensor dy = at::empty_like(y), dmu = at::empty_like(y);
  check_rc(ic_ckbd_input_bwd(y.data_ptr<float>(), mu.data_ptr<float>(), du.data_ptr<float>(), dv.data_ptr<float>(),
                             CKBD_DIMS(y), dy.data_ptr<float>(), dmu.data_ptr<float>(), stream_of(y)),
           "ckbd_input_bwd");
  return {dy, dmu};
}

std::tuple<Tensor, Tensor> ckbd_params_fwd(const Tensor& mu_h, const Tensor& sigma_h, const Tensor& a, const Tensor& b) {
  check_ckbd(mu_h, "mu_h");
  check_ckbd_like(mu_h, sigma_h, "sigma_h");
  check_ckbd_like(mu_h, a, "a");
  check_ckbd_like(mu_h, b, "b");
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(mu_h.device());
  Tensor mu = at::empty_like(mu_h), sigma = at::empty_like(mu_h);
  check_rc(ic_ckbd_params_fwd(mu_h.data_ptr<float>(), sigma_h.data_ptr<float>(), a.data_ptr<float>(), b.data_ptr<float>(),
                              CKBD_DIMS(mu_h), mu.data_ptr<float>(), sigma.data_ptr<float>(), stream_of(mu_h)),
           "ckbd_params_fwd");
  return {mu, sigma};
}

std::tuple<Tensor, Tensor, Tensor, Tensor> ckbd_params_bwd(const Tensor& sigma_h, const Tensor& b, const Tensor& dmu,
                                                           const Tensor& dsigma) {
  check_ckbd(sigma_h, "sigma_h");
  check_ckbd_like(sigma_h, b, "b");
  check_ckbd_like(sigma_h, dmu, "dmu");
  check_ckbd_like(sigma_h, dsigma, "dsigma");
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(sigma_h.device());
  Tensor dmu_h = at::empty_like(b), dsigma_h = at::empty_like(b), da = at::empty_like(b), db = at::empty_like(b);
  check_rc(ic_ckbd_params_bwd(sigma_h.data_ptr<float>(), b.data_ptr<float>(), dmu.data_ptr<float>(),
                              dsigma.data_ptr<float>(), CKBD_DIMS(b), dmu_h.data_ptr<float>(), dsigma_h.data_ptr<float>(),
                              da.data_ptr<float>(), db.data_ptr<float>(), stream_of(b)),
           "ckbd_params_bwd");
  return {dmu_h, dsigma_h, da, db};
}

// src uint8 (table rows), int32 (symbols) or float32
Tensor ckbd_gather(const Tensor& src, int64_t parity) {
  TORCH_CHECK(src.is_cuda(), "imgcomp_ckbd: src must be on a ROCm device, got ", src.device());
  const auto ty = src.scalar_type();
  TORCH_CHECK(ty == at::kByte || ty == at::kInt || ty == at::kFloat, "imgcomp_ckbd: src must be uint8, int32 or float32, got ",
              ty);
  check_ckbd_shape(src, "src");
  check_parity(parity);
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(src.device());
  Tensor half = at::empty({ckbd_half_numel(src, parity)}, src.options());
  if (half.numel() == 0) return half;   // a 1 x 1 map has no non-anchor
  check_rc(ic_ckbd_gather(src.data_ptr(), (int)src.element_size(), CKBD_DIMS(src), (int)parity, half.data_ptr(),
                          stream_of(src)),
           "ckbd_gather");
  return half;
}

void ckbd_scatter(const Tensor& half, Tensor& full, int64_t parity) {
  check_ckbd(full, "full");
  check_operand(half, "half");
  check_parity(parity);
  TORCH_CHECK(half.is_contiguous() && half.device() == full.device() && half.numel() == ckbd_half_numel(full, parity),
              "imgcomp_ckbd: the half (", half.numel(), " values) must be contiguous, on full's device and hold its ",
              ckbd_half_numel(full, parity), " values of parity ", parity);
  if (half.numel() == 0) return;
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(full.device());
  check_rc(ic_ckbd_scatter(half.data_ptr<float>(), CKBD_DIMS(full), (int)parity, full.data_ptr<float>(), stream_of(full)),
           "ckbd_scatter");
}

void check_ckbd_meta(const Tensor& a, std::initializer_list<const Tensor*> rest) {
  check_ckbd_shape(a, "the first operand");
  for (const Tensor* t : rest)
    TORCH_CHECK(t->sizes() == a.sizes(), "imgcomp_ckbd: operands must have the same shape, got ", a.sizes(), " and ",
                t->sizes());
}
std::tuple<Tensor, Tensor> ckbd_input_fwd_meta(const Tensor& y, const Tensor& mu) {
  check_ckbd_meta(y, {&mu});
  return {at::empty_like(y), at::empty_like(y)};
}
std::tuple<Tensor, Tensor> ckbd_input_bwd_meta(const Tensor& y, const Tensor& mu, const Tensor& du, const Tensor& dv) {
  check_ckbd_meta(y, {&mu, &du, &dv});
  return {at::empty_like(y), at::empty_like(y)};
}
std::tuple<Tensor, Tensor> ckbd_params_fwd_meta(const Tensor& mu_h, const Tensor& sigma_h, const Tensor& a, const Tensor& b) {
  check_ckbd_meta(mu_h, {&sigma_h, &a, &b});
  return {at::empty_like(mu_h), at::empty_like(mu_h)};
}
std::tuple<Tensor, Tensor, Tensor, Tensor> ckbd_params_bwd_meta(const Tensor& sigma_h, const Tensor& b, const Tensor& dmu,
                                                                const Tensor& dsigma) {
  check_ckbd_meta(sigma_h, {&b, &dmu, &dsigma});
  return {at::empty_like(b), at::empty_like(b), at::empty_like(b), at::empty_like(b)};
}
Tensor ckbd_gather_meta(const Tensor& src, int64_t parity) {
  check_ckbd_shape(src, "src");
  check_parity(parity);
  return at::empty({ckbd_half_numel(src, parity)}, src.options());
}
void ckbd_scatter_meta(const Tensor& half, Tensor& full, int64_t parity) {
  check_ckbd_shape(full, "full");
  check_parity(parity);
  TORCH_CHECK(half.numel() == ckbd_half_numel(full, parity), "imgcomp_ckbd: the half (", half.numel(),
              " values) must hold full's ", ckbd_half_numel(full, parity), " values of parity ", parity);
}

// ---------------------------------------------------------------- the context in one launch (imgcomp_ctx)
// y_in, mu_h, sigma_h as imgcomp_ckbd's full tensors; the weights (C, C, 5, 5) and biases (C) as Conv2d holds them.
void check_ctx_weights(int64_t C, const Tensor& w, const Tensor& b, const char* head, bool device) {
  if (device) {
    check_operand(w, head);
    check_operand(b, head);
  }
  TORCH_CHECK(w.dim() == 4 && w.size(0) == C && w.size(1) == C && w.size(2) == 5 && w.size(3) == 5 && w.is_contiguous(),
              "imgcomp_ctx: the ", head, " weight must be a contiguous (", C, ", ", C, ", 5, 5) tensor, got ", w.sizes());
  TORCH_CHECK(b.dim() == 1 && b.size(0) == C && b.is_contiguous(), "imgcomp_ctx: the ", head, " bias must be (", C,
              "), got ", b.sizes());
}

std::tuple<Tensor, Tensor> ctx_launch(const Tensor& y_in, const Tensor& mu_h, const Tensor& sigma_h, const Tensor& w_mean,
                                      const Tensor& b_mean, const Tensor& w_scale, const Tensor& b_scale, Tensor* own_ws,
                                      bool packed) {
  check_ckbd(y_in, "y_in");
  check_ckbd_like(y_in, mu_h, "mu_h");
  check_ckbd_like(y_in, sigma_h, "sigma_h");
  const int64_t C = y_in.size(3);
  check_ctx_weights(C, w_mean, b_mean, "mean", true);
  check_ctx_weights(C, w_scale, b_scale, "scale", true);
  for (const Tensor* t : {&w_mean, &b_mean, &w_scale, &b_scale})
    TORCH_CHECK(t->device() == y_in.device(), "imgcomp_ctx: the weights must be on y_in's device");
  const size_t nb = ic_context_ws((int)std::min<int64_t>(C, INT_MAX));
  TORCH_CHECK(nb > 0, "imgcomp_ctx: ", C, " channels (1 .. ", IC_CONTEXT_MAXC, ")");
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(y_in.device());
  Tensor ws;
  if (own_ws) {
    TORCH_CHECK(own_ws->is_cuda() && own_ws->scalar_type() == at::kByte && own_ws->is_contiguous() &&
                    own_ws->device() == y_in.device(),
                "imgcomp_ctx: ws must be a contiguous uint8 tensor on y_in's device");
    if ((size_t)own_ws->numel() < nb) {
      TORCH_CHECK(!packed, "imgcomp_ctx: packed weights expected in a workspace of ", own_ws->numel(), " bytes, the op needs ",
                  nb);
      own_ws->resize_({(int64_t)nb});
    }
    ws = *own_ws;
  } else {
    ws = workspace(y_in, nb);
  }
  Tensor mu = at::empty_like(y_in), sigma = at::empty_like(y_in);
  check_rc(ic_context_fwd(y_in.data_ptr<float>(), mu_h.data_ptr<float>(), sigma_h.data_ptr<float>(),
                               w_mean.data_ptr<float>(), b_mean.data_ptr<float>(), w_scale.data_ptr<float>(),
                               b_scale.data_ptr<float>(), CKBD_DIMS(y_in), mu.data_ptr<float>(), sigma.data_ptr<float>(),
                               ws.data_ptr(), (size_t)ws.numel(), packed ? 1 : 0, stream_of(y_in)),
           "context_fwd");
  return {mu, sigma};
}

std::tuple<Tensor, Tensor> ctx_context_fwd(const Tensor& y_in, const Tensor& mu_h, const Tensor& sigma_h,
                                           const Tensor& w_mean, const Tensor& b_mean, const Tensor& w_scale,
                                           const Tensor& b_scale) {
  return ctx_launch(y_in, mu_h, sigma_h, w_mean, b_mean, w_scale, b_scale, nullptr, false);
}

// the packed weights kept by the caller: written to `ws` (grown when too small), or with `packed` read from it
std::tuple<Tensor, Tensor> ctx_context_fwd_ws(const Tensor& y_in, const Tensor& mu_h, const Tensor& sigma_h,
                                              const Tensor& w_mean, const Tensor& b_mean, const Tensor& w_scale,
                                              const Tensor& b_scale, Tensor& ws, bool packed) {
  return ctx_launch(y_in, mu_h, sigma_h, w_mean, b_mean, w_scale, b_scale, &ws, packed);
}

std::tuple<Tensor, Tensor> ctx_context_fwd_meta(const Tensor& y_in, const Tensor& mu_h, const Tensor& sigma_h,
                                                const Tensor& w_mean, const Tensor& b_mean, const Tensor& w_scale,
                                                const Tensor& b_scale) {
  check_ckbd_meta(y_in, {&mu_h, &sigma_h});
  check_ctx_weights(y_in.size(3), w_mean, b_mean, "mean", false);
  check_ctx_weights(y_in.size(3), w_scale, b_scale, "scale", false);
  return {at::empty_like(y_in), at::empty_like(y_in)};
}
std::tuple<Tensor, Tensor> ctx_context_fwd_ws_meta(const Tensor& y_in, const Tensor& mu_h, const Tensor& sigma_h,
                                                   const Tensor& w_mean, const Tensor& b_mean, const Tensor& w_scale,
                                                   const Tensor& b_scale, Tensor& ws, bool packed) {
  return ctx_context_fwd_meta(y_in, mu_h, sigma_h, w_mean, b_mean, w_scale, b_scale);
}

// ---------------------------------------------------------------- h_s as batch-invariant layers (imgcomp_hs)
// x: (N, H, W, Cin) dense channels-last storage; w: (Cin, Cout, k, k) and b: (Cout) as ConvTranspose2d holds them.
// Returns (out, out2), out2 with no element when there is no second head.
struct HsShape {
  int64_t N, H, W, Cin, Cout, k, heads;
};

HsShape check_hs(const Tensor& x, const Tensor& w, const Tensor& b, int64_t stride, int64_t epilogue,
                 const c10::optional<Tensor>& w2, const c10::optional<Tensor>& b2, int64_t epilogue2, bool device) {
  TORCH_CHECK(x.dim() == 4 && x.is_contiguous() && x.numel() > 0, "imgcomp_hs: x must be a contiguous, non-empty "
              "(N, H, W, C) tensor, got ", x.sizes());
  for (int64_t d = 0; d < 4; ++d) TORCH_CHECK(x.size(d) <= INT_MAX / 2, "imgcomp_hs: x is too large: ", x.sizes());
  TORCH_CHECK(w.dim() == 4 && w.is_contiguous() && w.size(0) == x.size(3) && w.size(2) == w.size(3) && w.size(1) >= 1,
              "imgcomp_hs: the weight must be a contiguous (", x.size(3), ", Cout, k, k) tensor, got ", w.sizes());
  HsShape g{x.size(0), x.size(1), x.size(2), x.size(3), w.size(1), w.size(2), 1};
  TORCH_CHECK(b.dim() == 1 && b.size(0) == g.Cout && b.is_contiguous(), "imgcomp_hs: the bias must be (", g.Cout,
              "), got ", b.sizes());
  const bool second = w2.has_value() && w2->defined();
  TORCH_CHECK(second == (b2.has_value() && b2->defined()), "imgcomp_hs: the second head needs a weight and a bias");
  if (second) {
    g.heads = 2;
    TORCH_CHECK(w2->sizes() == w.sizes() && w2->is_contiguous() && b2->sizes() == b.sizes() && b2->is_contiguous(),
                "imgcomp_hs: the second head's weight ", w2->sizes(), " and bias ", b2->sizes(),
                " must be contiguous and shaped as the first's, ", w.sizes(), " and ", b.sizes());
  }
  TORCH_CHECK(g.Cin <= INT_MAX && g.Cout <= INT_MAX && g.k <= INT_MAX &&
                  ic_hs_ws((int)g.Cin, (int)g.Cout, (int)g.k, (int)std::min<int64_t>(std::max<int64_t>(stride, 0), 3),
                           (int)g.heads) > 0,
              "imgcomp_hs: no kernel for k ", g.k, ", stride ", stride, ", channels ", g.Cin, " -> ", g.Cout,
              " (k odd and <= 5, stride 1 or 2, 1 .. ", IC_HS_MAXC, " channels)");
  for (int64_t e : {epilogue, second ? epilogue2 : (int64_t)IC_HS_NONE})
    TORCH_CHECK(e == IC_HS_NONE || e == IC_HS_RELU || e == IC_HS_EXP_CLAMP, "imgcomp_hs: no epilogue ", e);
  if (device) {
    check_operand(x, "x");
    for (const Tensor* t : {&w, &b, second ? &*w2 : &w, second ? &*b2 : &b}) {
      check_operand(*t, "a weight or bias");
      TORCH_CHECK(t->device() == x.device(), "imgcomp_hs: the weights must be on x's device");
    }
  } else {
    TORCH_CHECK(x.scalar_type() == at::kFloat && w.scalar_type() == at::kFloat && b.scalar_type() == at::kFloat,
                "imgcomp_hs: operands must be float32");
  }
  return g;
}

std::tuple<Tensor, Tensor> hs_launch(const Tensor& x, const Tensor& w, const Tensor& b, int64_t stride, int64_t epilogue,
                                     const c10::optional<Tensor>& w2, const c10::optional<Tensor>& b2,
                                     int64_t epilogue2, double lo, double hi, Tensor* own_ws, bool packed) {
  const HsShape g = check_hs(x, w, b, stride, epilogue, w2, b2, epilogue2, true);
  const size_t nb = ic_hs_ws((int)g.Cin, (int)g.Cout, (int)g.k, (int)stride, (int)g.heads);
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(x.device());
  Tensor ws;
  if (own_ws) {
    TORCH_CHECK(own_ws->is_cuda() && own_ws->scalar_type() == at::kByte && own_ws->is_contiguous() &&
                    own_ws->device() == x.device(),
                "imgcomp_hs: ws must be a contiguous uint8 tensor on x's device");
    if ((size_t)own_ws->numel() < nb) {
      TORCH_CHECK(!packed, "imgcomp_hs: packed weights expected in a workspace of ", own_ws->numel(),
                  " bytes, the op needs ", nb);
      own_ws->resize_({(int64_t)nb});
    }
    ws = *own_ws;
  } else {
    ws = workspace(x, nb);
  }
  Tensor out = at::empty({g.N, stride * g.H, stride * g.W, g.Cout}, x.options());
  Tensor out2 = g.heads == 2 ? at::empty_like(out) : at::empty({0}, x.options());
  check_rc(ic_hs_layer(x.data_ptr<float>(), (int)g.N, (int)g.H, (int)g.W, (int)g.Cin, (int)g.Cout, (int)g.k, (int)stride,
                       w.data_ptr<float>(), b.data_ptr<float>(), (int)epilogue, out.data_ptr<float>(),
                       g.heads == 2 ? w2->data_ptr<float>() : nullptr, g.heads == 2 ? b2->data_ptr<float>() : nullptr,
                       g.heads == 2 ? (int)epilogue2 : 0, g.heads == 2 ? out2.data_ptr<float>() : nullptr, (float)lo,
                       (float)hi, ws.data_ptr(), (size_t)ws.numel(), packed ? 1 : 0, stream_of(x)),
           "hs layer");
  return {out, out2};
}

std::tuple<Tensor, Tensor> hs_layer(const Tensor& x, const Tensor& w, const Tensor& b, int64_t stride, int64_t epilogue,
                                    const c10::optional<Tensor>& w2, const c10::optional<Tensor>& b2, int64_t epilogue2,
                                    double lo, double hi) {
  return hs_launch(x, w, b, stride, epilogue, w2, b2, epilogue2, lo, hi, nullptr, false);
}

// the packed weights kept by the caller: written to `ws` (grown when too small), or with `packed` read from it
std::tuple<Tensor, Tensor> hs_layer_ws(const Tensor& x, const Tensor& w, const Tensor& b, int64_t stride,
                                       int64_t epilogue, const c10::optional<Tensor>& w2,
                                       const c10::optional<Tensor>& b2, int64_t epilogue2, double lo, double hi,
                                       Tensor& ws, bool packed) {
  return hs_launch(x, w, b, stride, epilogue, w2, b2, epilogue2, lo, hi, &ws, packed);
}

std::tuple<Tensor, Tensor> hs_layer_meta(const Tensor& x, const Tensor& w, const Tensor& b, int64_t stride,
                                         int64_t epilogue, const c10::optional<Tensor>& w2,
                                         const c10::optional<Tensor>& b2, int64_t epilogue2, double lo, double hi) {
  const HsShape g = check_hs(x, w, b, stride, epilogue, w2, b2, epilogue2, false);
  Tensor out = at::empty({g.N, stride * g.H, stride * g.W, g.Cout}, x.options());
  return {out, g.heads == 2 ? at::empty_like(out) : at::empty({0}, x.options())};
}
std::tuple<Tensor, Tensor> hs_layer_ws_meta(const Tensor& x, const Tensor& w, const Tensor& b, int64_t stride,
                                            int64_t epilogue, const c10::optional<Tensor>& w2,
                                            const c10::optional<Tensor>& b2, int64_t epilogue2, double lo, double hi,
                                            Tensor& ws, bool packed) {
  return hs_layer_meta(x, w, b, stride, epilogue, w2, b2, epilogue2, lo, hi);
}

// ---------------------------------------------------------------- gain units (imgcomp_gain)
// A level table is (S, C); a set of gain vectors (rows, C), one row per quality; a latent is a contiguous
// (N, *, C) tensor, the channels-last storage the coder flattens, scaled by row 0 (rows == 1) or by row n.
std::vector<float> check_qualities(c10::ArrayRef<double> q, int64_t S) {
  TORCH_CHECK_VALUE(S >= 2, "imgcomp_gain: a level table has at least 2 levels, got ", S);
  TORCH_CHECK_VALUE(!q.empty() && q.size() <= (size_t)INT_MAX, "imgcomp_gain: ", q.size(), " qualities");
  std::vector<float> out;
  for (double v : q) {
    TORCH_CHECK_VALUE(v >= 0.0 && v <= (double)(S - 1), "imgcomp_gain: quality ", v, " is outside [0, ", S - 1, "]");
    out.push_back((float)v);
  }
  return out;
}

void check_gain_matrix(const Tensor& t, const char* what) {
  check_operand(t, what);
  TORCH_CHECK(t.dim() == 2 && t.is_contiguous() && t.size(0) >= 1 && t.size(1) >= 1 && t.numel() <= INT_MAX,
              "imgcomp_gain: ", what, " must be a non-empty contiguous 2-D tensor, got ", t.sizes());
}

void check_scale_shapes(const Tensor& x, const Tensor& g) {
  TORCH_CHECK(x.dim() >= 2 && x.is_contiguous() && x.numel() > 0, "imgcomp_gain: x must be a non-empty contiguous "
              "(N, *, C) tensor, got ", x.sizes());
  TORCH_CHECK(g.dim() == 2 && g.is_contiguous() && g.size(1) == x.size(-1) && (g.size(0) == 1 || g.size(0) == x.size(0)),
              "imgcomp_gain: the gains ", g.sizes(), " must be contiguous (1 or N, C) for x ", x.sizes());
  TORCH_CHECK(x.size(0) <= 65535 && x.size(-1) <= INT_MAX, "imgcomp_gain: x is too large: ", x.sizes());
}

void check_scale(const Tensor& x, const Tensor& g) {
  check_operand(x, "x");
  check_operand(g, "g");
  check_scale_shapes(x, g);
  TORCH_CHECK(x.device() == g.device(), "imgcomp_gain: x and g must be on one device");
}

Tensor gain_vector(const Tensor& table, c10::ArrayRef<double> q) {
  check_gain_matrix(table, "table");
  const std::vector<float> qs = check_qualities(q, table.size(0));
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(table.device());
  Tensor out = at::empty({(int64_t)qs.size(), table.size(1)}, table.options());
  check_rc(ic_gain_vector(table.data_ptr<float>(), (int)table.size(0), (int)table.size(1), qs.data(), (int)qs.size(),
                          out.data_ptr<float>(), stream_of(table)),
           "gain_vector");
  return out;
}

Tensor gain_vector_bwd(const Tensor& g, const Tensor& dout, int64_t S, c10::ArrayRef<double> q) {
  check_gain_matrix(g, "g");
  check_gain_matrix(dout, "dout");
  const std::vector<float> qs = check_qualities(q, S);
  TORCH_CHECK(g.sizes() == dout.sizes() && g.device() == dout.device() && g.size(0) == (int64_t)qs.size(),
              "imgcomp_gain: g ", g.sizes(), " and dout ", dout.sizes(), " must be (", qs.size(), ", C) on one device");
  TORCH_CHECK(S * g.size(1) <= INT_MAX, "imgcomp_gain: the table is too large");
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(g.device());
  Tensor dtable = at::empty({S, g.size(1)}, g.options());
  check_rc(ic_gain_vector_bwd(g.data_ptr<float>(), dout.data_ptr<float>(), (int)S, (int)g.size(1), qs.data(),
                              (int)qs.size(), dtable.data_ptr<float>(), stream_of(g)),
           "gain_vector_bwd");
  return dtable;
}

Tensor channel_scale(const Tensor& x, const Tensor& g) {
  check_scale(x, g);
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(x.device());
  Tensor out = at::empty_like(x);
  const int64_t N = x.size(0), C = x.size(-1);
  check_rc(ic_channel_scale(x.data_ptr<float>(), g.data_ptr<float>(), N, x.numel() / N / C, (int)C, (int)g.size(0),
                            out.data_ptr<float>(), stream_of(x)),
           "channel_scale");
  return out;
}

std::tuple<Tensor, Tensor> channel_scale_bwd(const Tensor& x, const Tensor& g, const Tensor& dy) {
  check_scale(x, g);
  check_operand(dy, "dy");
  TORCH_CHECK(dy.sizes() == x.sizes() && dy.is_contiguous() && dy.device() == x.device(), "imgcomp_gain: dy ", dy.sizes(),
              " must be contiguous with the shape ", x.sizes(), " of x, on its device");
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(x.device());
  Tensor dx = at::empty_like(x), dg = at::empty_like(g);
  const int64_t N = x.size(0), C = x.size(-1), P = x.numel() / N / C;
  const size_t nb = ic_channel_scale_bwd_ws(N, P, (int)C, (int)g.size(0));
  Tensor ws = workspace(x, nb);
  check_rc(ic_channel_scale_bwd(x.data_ptr<float>(), g.data_ptr<float>(), dy.data_ptr<float>(), N, P, (int)C,
                                (int)g.size(0), dx.data_ptr<float>(), dg.data_ptr<float>(), ws.data_ptr(), nb,
                                stream_of(x)),
           "channel_scale_bwd");
  return {dx, dg};
}

Tensor gain_vector_meta(const Tensor& table, c10::ArrayRef<double> q) {
  TORCH_CHECK(table.dim() == 2, "imgcomp_gain: table must be (S, C), got ", table.sizes());
  check_qualities(q, table.size(0));
  return at::empty({(int64_t)q.size(), table.size(1)}, table.options());
}
Tensor gain_vector_bwd_meta(const Tensor& g, const Tensor& dout, int64_t S, c10::ArrayRef<double> q) {
  check_qualities(q, S);
  TORCH_CHECK(g.dim() == 2 && g.sizes() == dout.sizes() && g.size(0) == (int64_t)q.size(), "imgcomp_gain: g ", g.sizes(),
              " and dout ", dout.sizes(), " must be (", q.size(), ", C)");
  return at::empty({S, g.size(1)}, g.options());
}
Tensor channel_scale_meta(const Tensor& x, const Tensor& g) {
  check_scale_shapes(x, g);
  return at::empty_like(x);
}
std::tuple<Tensor, Tensor> channel_scale_bwd_meta(const Tensor& x, const Tensor& g, const Tensor& dy) {
  check_scale_shapes(x, g);
  TORCH_CHECK(dy.sizes() == x.sizes(), "imgcomp_gain: dy ", dy.sizes(), " must have the shape ", x.sizes(), " of x");
  return {at::empty_like(x), at::empty_like(g)};
}

// ---------------------------------------------------------------- region-of-interest coding (imgcomp_region)
// A latent is a contiguous (N, Hm, Wm, C) tensor; the gains (R, C); a block map a contiguous uint8 tensor
// (N, ceil(Hm / 2^shift), ceil(Wm / 2^shift)) of ranks below R.  An image pair is (N, C, H, W) with shared strides,
// its map (N, ceil(H / 64), ceil(W / 64)), its weights (R).
int64_t map_extent(int64_t v, int64_t shift) { return (v + (int64_t(1) << shift) - 1) >> shift; }

void check_region_shapes(const Tensor& x, const Tensor& g, const Tensor& idx, int64_t shift) {
  TORCH_CHECK_VALUE(shift >= 0 && shift <= 6, "imgcomp_region: a block is 2^shift positions wide, shift in 0 .. 6, got ",
                    shift);
  TORCH_CHECK(x.dim() == 4 && x.is_contiguous() && x.numel() > 0, "imgcomp_region: x must be a non-empty contiguous "
              "(N, Hm, Wm, C) tensor, got ", x.sizes());
  TORCH_CHECK(g.dim() == 2 && g.is_contiguous() && g.size(1) == x.size(3) && g.size(0) >= 1 && g.size(0) <= 256,
              "imgcomp_region: the gains ", g.sizes(), " must be contiguous (1 .. 256, C) for x ", x.sizes());
  TORCH_CHECK(x.size(0) <= 65535 && x.numel() / x.size(0) <= INT_MAX, "imgcomp_region: x is too large: ", x.sizes());
  TORCH_CHECK(idx.scalar_type() == at::kByte && idx.dim() == 3 && idx.is_contiguous() && idx.size(0) == x.size(0) &&
                  idx.size(1) == map_extent(x.size(1), shift) && idx.size(2) == map_extent(x.size(2), shift),
              "imgcomp_region: the block map ", idx.sizes(), " must be contiguous uint8 (", x.size(0), ", ",
              map_extent(x.size(1), shift), ", ", map_extent(x.size(2), shift), ") for x ", x.sizes(), " at shift ", shift);
}

void check_region(const Tensor& x, const Tensor& g, const Tensor& idx, int64_t shift) {
  check_operand(x, "x");
  check_operand(g, "g");
  TORCH_CHECK(idx.is_cuda(), "imgcomp: the block map must be on a ROCm device, got ", idx.device());
  check_region_shapes(x, g, idx, shift);
  TORCH_CHECK(x.device() == g.device() && x.device() == idx.device(), "imgcomp_region: x, g and the block map must be on "
              "one device");
}

Tensor block_scale(const Tensor& x, const Tensor& g, const Tensor& idx, int64_t shift) {
  check_region(x, g, idx, shift);
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(x.device());
  Tensor out = at::empty_like(x);
  check_rc(ic_block_scale(x.data_ptr<float>(), g.data_ptr<float>(), (int)g.size(0), idx.data_ptr<uint8_t>(), (int)x.size(0),
                          (int)x.size(1), (int)x.size(2), (int)x.size(3), (int)shift, out.data_ptr<float>(), stream_of(x)),
           "block_scale");
  return out;
}

std::tuple<Tensor, Tensor> block_scale_bwd(const Tensor& x, const Tensor& g, const Tensor& idx, const Tensor& dy,
                                           int64_t shift) {
  check_region(x, g, idx, shift);
  check_operand(dy, "dy");
  TORCH_CHECK(dy.sizes() == x.sizes() && dy.is_contiguous() && dy.device() == x.device(), "imgcomp_region: dy ",
              dy.sizes(), " must be contiguous with the shape ", x.sizes(), " of x, on its device");
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(x.device());
  Tensor dx = at::empty_like(x), dg = at::empty_like(g);
  const int N = (int)x.size(0), Hm = (int)x.size(1), Wm = (int)x.size(2), C = (int)x.size(3);
  const size_t nb = ic_block_scale_bwd_ws(N, Hm, Wm, C, (int)shift);
  Tensor ws = workspace(x, nb);
  check_rc(ic_block_scale_bwd(x.data_ptr<float>(), g.data_ptr<float>(), (int)g.size(0), idx.data_ptr<uint8_t>(),
                              dy.data_ptr<float>(), N, Hm, Wm, C, (int)shift, dx.data_ptr<float>(), dg.data_ptr<float>(),
                              ws.data_ptr(), nb, stream_of(x)),
           "block_scale_bwd");
  return {dx, dg};
}

void check_block_mse_shapes(const Tensor& a, const Tensor& b, const Tensor& w, const Tensor& idx) {
  TORCH_CHECK(a.dim() == 4 && a.numel() > 0 && a.is_non_overlapping_and_dense(), "imgcomp_region: the images must be "
              "non-empty dense (N, C, H, W) tensors, got ", a.sizes());
  TORCH_CHECK(b.sizes() == a.sizes() && b.strides() == a.strides(), "imgcomp_region: the two images must share shape "
              "and strides: ", a.sizes(), " / ", a.strides(), " and ", b.sizes(), " / ", b.strides());
  TORCH_CHECK(a.size(0) <= 65535 && a.numel() / a.size(0) <= INT_MAX, "imgcomp_region: the images are too large: ",
              a.sizes());
  TORCH_CHECK(w.dim() == 1 && w.is_contiguous() && w.size(0) >= 1 && w.size(0) <= 256, "imgcomp_region: the weights ",
              w.sizes(), " must be a contiguous vector of 1 .. 256");
  TORCH_CHECK(idx.scalar_type() == at::kByte && idx.dim() == 3 && idx.is_contiguous() && idx.size(0) == a.size(0) &&
                  idx.size(1) == map_extent(a.size(2), 6) && idx.size(2) == map_extent(a.size(3), 6),
              "imgcomp_region: the block map ", idx.sizes(), " must be contiguous uint8 (", a.size(0), ", ",
              map_extent(a.size(2), 6), ", ", map_extent(a.size(3), 6), ") for images ", a.sizes());
}

void check_block_mse(const Tensor& a, const Tensor& b, const Tensor& w, const Tensor& idx) {
  check_operand(a, "input");
  check_operand(b, "target");
  check_operand(w, "the weights");
  TORCH_CHECK(idx.is_cuda(), "imgcomp: the block map must be on a ROCm device, got ", idx.device());
  check_block_mse_shapes(a, b, w, idx);
  TORCH_CHECK(a.device() == b.device() && a.device() == w.device() && a.device() == idx.device(),
              "imgcomp_region: the images, the weights and the block map must be on one device");
}

// {weighted mean, plain mean} of the squared error
Tensor block_mse_fwd(const Tensor& a, const Tensor& b, const Tensor& w, const Tensor& idx) {
  check_block_mse(a, b, w, idx);
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(a.device());
  Tensor out = at::empty({2}, a.options().memory_format(at::MemoryFormat::Contiguous));
  const int N = (int)a.size(0), C = (int)a.size(1), H = (int)a.size(2), W = (int)a.size(3);
  const size_t nb = ic_block_mse_ws(N, C, H, W);
  Tensor ws = workspace(a, nb);
  check_rc(ic_block_mse_fwd(a.data_ptr<float>(), b.data_ptr<float>(), w.data_ptr<float>(), (int)w.size(0),
                            idx.data_ptr<uint8_t>(), N, C, H, W, a.stride(0), a.stride(1), a.stride(2), a.stride(3),
                            out.data_ptr<float>(), ws.data_ptr(), nb, stream_of(a)),
           "block_mse_fwd");
  return out;
}

// (ga, gb); a gradient that is not wanted comes back empty (0 elements)
std::tuple<Tensor, Tensor> block_mse_bwd(const Tensor& a, const Tensor& b, const Tensor& w, const Tensor& idx,
                                         const Tensor& g, bool need_a, bool need_b) {
  check_block_mse(a, b, w, idx);
  check_operand(g, "gradient");
  TORCH_CHECK(g.numel() == 1, "block_mse_bwd: the gradient of a scalar loss is one value");
  TORCH_CHECK(need_a || need_b, "block_mse_bwd: no gradient is asked for");
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(a.device());
  Tensor gc = g.contiguous();
  Tensor ga = need_a ? at::empty_strided(a.sizes(), a.strides(), a.options()) : at::empty({0}, a.options());
  Tensor gb = need_b ? at::empty_strided(a.sizes(), a.strides(), a.options()) : at::empty({0}, a.options());
  check_rc(ic_block_mse_bwd(a.data_ptr<float>(), b.data_ptr<float>(), w.data_ptr<float>(), (int)w.size(0),
                            idx.data_ptr<uint8_t>(), gc.data_ptr<float>(), (int)a.size(0), (int)a.size(1), (int)a.size(2),
                            (int)a.size(3), a.stride(0), a.stride(1), a.stride(2), a.stride(3),
                            need_a ? ga.data_ptr<float>() : nullptr, need_b ? gb.data_ptr<float>() : nullptr, stream_of(a)),
           "block_mse_bwd");
  return {ga, gb};
}

Tensor block_scale_meta(const Tensor& x, const Tensor& g, const Tensor& idx, int64_t shift) {
  check_region_shapes(x, g, idx, shift);
  return at::empty_like(x);
}
std::tuple<Tensor, Tensor> block_scale_bwd_meta(const Tensor& x, const Tensor& g, const Tensor& idx, const Tensor& dy,
                                                int64_t shift) {
  check_region_shapes(x, g, idx, shift);
  TORCH_CHECK(dy.sizes() == x.sizes(), "imgcomp_region: dy ", dy.sizes(), " must have the shape ", x.sizes(), " of x");
  return {at::empty_like(x), at::empty_like(g)};
}
Tensor block_mse_fwd_meta(const Tensor& a, const Tensor& b, const Tensor& w, const Tensor& idx) {
  check_block_mse_shapes(a, b, w, idx);
  return at::empty({2}, a.options().memory_format(at::MemoryFormat::Contiguous));
}
std::tuple<Tensor, Tensor> block_mse_bwd_meta(const Tensor& a, const Tensor& b, const Tensor& w, const Tensor& idx,
                                              const Tensor& g, bool need_a, bool need_b) {
  check_block_mse_shapes(a, b, w, idx);
  return {need_a ? at::empty_strided(a.sizes(), a.strides(), a.options()) : at::empty({0}, a.options()),
          need_b ? at::empty_strided(a.sizes(), a.strides(), a.options()) : at::empty({0}, a.options())};
}

// ---------------------------------------------------------------- rate and distortion maps (imgcomp_map)
// A tensor is the logical (N, C, H, W); inside an image its storage is dense channels-last or dense NCHW (the stride
// of an extent of 1 is not looked at).  A map is contiguous (N, ceil(H / 2^shift), ceil(W / 2^shift)).  Inference
// only: no autograd node.
bool map_layout_ok(const Tensor& t) {
  const int64_t C = t.size(1), H = t.size(2), W = t.size(3), sc = t.stride(1), sh = t.stride(2), sw = t.stride(3);
  const bool last = (C == 1 || sc == 1) && (W == 1 || sw == C) && (H == 1 || sh == W * C);
  const bool nchw = (W == 1 || sw == 1) && (H == 1 || sh == W) && (C == 1 || sc == H * W);
  return last || nchw;
}

void check_map_shapes(const Tensor& t, int64_t shift, const char* what) {
  TORCH_CHECK_VALUE(shift >= 0 && shift <= 6, "imgcomp_map: a block is 2^shift positions wide, shift in 0 .. 6, got ",
                    shift);
  TORCH_CHECK(t.dim() == 4 && t.numel() > 0, "imgcomp_map: ", what, " must be a non-empty (N, C, H, W) tensor, got ",
              t.sizes());
  TORCH_CHECK(t.size(0) <= 65535 && t.numel() / t.size(0) <= INT_MAX, "imgcomp_map: ", what, " is too large: ", t.sizes());
}

void check_map_operand(const Tensor& t, const char* what) {
  check_operand(t, what);
  TORCH_CHECK(map_layout_ok(t) && t.stride(0) >= 0, "imgcomp_map: every image of ", what, " must be dense channels-last "
              "or dense NCHW storage, got sizes ", t.sizes(), " with strides ", t.strides());
}

Tensor new_map(const Tensor& t, int64_t shift) {
  return at::empty({t.size(0), map_extent(t.size(2), shift), map_extent(t.size(3), shift)},
                   t.options().memory_format(at::MemoryFormat::Contiguous));
}

void check_map_add(const Tensor& p, int64_t shift, const std::optional<Tensor>& add) {
  if (!add.has_value() || !add->defined()) return;
  TORCH_CHECK(add->dim() == 3 && add->size(0) == p.size(0) && add->size(1) == map_extent(p.size(2), shift) &&
                  add->size(2) == map_extent(p.size(3), shift) && add->is_contiguous(),
              "imgcomp_map: add ", add->sizes(), " must be a contiguous map (", p.size(0), ", ",
              map_extent(p.size(2), shift), ", ", map_extent(p.size(3), shift), ") of p ", p.sizes(), " at shift ", shift);
}

Tensor map_block_bits(const Tensor& p, int64_t shift, const std::optional<Tensor>& add) {
  check_map_shapes(p, shift, "p");
  check_map_operand(p, "p");
  check_map_add(p, shift, add);
  if (add.has_value() && add->defined()) {
    check_operand(*add, "add");
    TORCH_CHECK(add->device() == p.device(), "imgcomp_map: p and add must be on one device");
  }
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(p.device());
  Tensor out = new_map(p, shift);
  check_rc(ic_block_bits(p.data_ptr<float>(), (int)p.size(0), (int)p.size(1), (int)p.size(2), (int)p.size(3), p.stride(0),
                         p.stride(1), p.stride(2), p.stride(3), (int)shift, opt_ptr(add), out.data_ptr<float>(),
                         stream_of(p)),
           "block_bits");
  return out;
}

Tensor map_block_sse(const Tensor& a, const Tensor& b, int64_t shift) {
  check_map_shapes(a, shift, "a");
  TORCH_CHECK(b.sizes() == a.sizes(), "imgcomp_map: the two images must share a shape, got ", a.sizes(), " and ",
              b.sizes());
  check_map_operand(a, "a");
  check_map_operand(b, "b");
  TORCH_CHECK(a.device() == b.device(), "imgcomp_map: the two images must be on one device");
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(a.device());
  Tensor out = new_map(a, shift);
  check_rc(ic_block_sse(a.data_ptr<float>(), b.data_ptr<float>(), (int)a.size(0), (int)a.size(1), (int)a.size(2),
                        (int)a.size(3), a.stride(0), a.stride(1), a.stride(2), a.stride(3), b.stride(0), b.stride(1),
                        b.stride(2), b.stride(3), (int)shift, out.data_ptr<float>(), stream_of(a)),
           "block_sse");
  return out;
}

Tensor map_block_bits_meta(const Tensor& p, int64_t shift, const std::optional<Tensor>& add) {
  check_map_shapes(p, shift, "p");
  check_map_add(p, shift, add);
  return new_map(p, shift);
}
Tensor map_block_sse_meta(const Tensor& a, const Tensor& b, int64_t shift) {
  check_map_shapes(a, shift, "a");
  TORCH_CHECK(b.sizes() == a.sizes(), "imgcomp_map: the two images must share a shape, got ", a.sizes(), " and ",
              b.sizes());
  return new_map(a, shift);
}

// ---------------------------------------------------------------- coding to a byte budget (imgcomp_rate)
// stream_encode_seg without its bytes: the chunk lengths, int32 (nseg * chunks per segment) on the device
Tensor rate_measure_seg(const Tensor& sym, int64_t nseg, const std::optional<Tensor>& rows, int64_t C, const Tensor& pool,
                        int64_t nrows, at::IntArrayRef seg_k, at::IntArrayRef seg_off, int64_t steps) {
  check_codec(sym, at::kInt, "sym");
  check_codec(pool, at::kInt, "table pool");
  const SegTables t = seg_tables(nseg, seg_k, seg_off);
  const int64_t n = sym.numel();
  TORCH_CHECK(n > 0 && n % nseg == 0, "imgcomp_rate: ", n, " symbols do not make ", nseg, " equal segments");
  const unsigned char* rp = codec_rows(rows, n);
  TORCH_CHECK(steps >= 1 && steps <= IC_CODEC_MAXR, "imgcomp_rate: steps_per_chunk in [1, ", IC_CODEC_MAXR, "]");
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(sym.device());
  const int64_t seg_len = n / nseg, chunks = ic_codec_seg_chunks((int)nseg, seg_len, (int)steps);
  TORCH_CHECK(chunks > 0, "imgcomp_rate: too many chunks");
  Tensor lens = at::empty({chunks}, sym.options());
  Tensor kt = at::empty({2 * nseg}, sym.options());
  check_rc(ic_codec_measure_seg(sym.data_ptr<int>(), (int)nseg, seg_len, rp, (int)C,
                                (const unsigned int*)pool.data_ptr<int>(), (size_t)pool.numel(), (int)nrows, t.k.data(),
                                t.off.data(), kt.data_ptr<int>(), (int)steps, (unsigned int*)lens.data_ptr<int>(),
                                stream_of(sym)),
           "codec_measure_seg");
  return lens;
}

// y (N, *, C) contiguous, read in place; g (M, C); mu: the M candidates' means back to back, each an image of y's
// size; img: the image of every candidate
void check_rate_shapes(const Tensor& y, const Tensor& g, const Tensor& mu, at::IntArrayRef img) {
  const int64_t M = (int64_t)img.size();
  TORCH_CHECK(y.dim() >= 2 && y.numel() > 0, "imgcomp_rate: y must be a non-empty (N, *, C) tensor, got ", y.sizes());
  TORCH_CHECK(M >= 1 && M <= 65535 && g.dim() == 2 && g.size(0) == M && g.size(1) == y.size(-1),
              "imgcomp_rate: the gains ", g.sizes(), " must be (", M, " candidates, ", y.size(-1), ")");
  TORCH_CHECK(mu.numel() == M * (y.numel() / y.size(0)), "imgcomp_rate: mu (", mu.numel(), " values) must hold ", M,
              " images of ", y.numel() / y.size(0), " values");
}

std::tuple<Tensor, std::vector<int64_t>> rate_gain_symbolize_seg(const Tensor& y, const Tensor& g, const Tensor& mu,
                                                                 at::IntArrayRef img) {
  check_operand(y, "y");
  check_operand(g, "g");
  check_operand(mu, "mu");
  check_rate_shapes(y, g, mu, img);
  TORCH_CHECK(y.is_contiguous() && g.is_contiguous() && mu.is_contiguous(), "imgcomp_rate: y, g and mu must be contiguous");
  TORCH_CHECK(y.device() == g.device() && y.device() == mu.device(), "imgcomp_rate: y, g and mu must be on one device");
  const int64_t M = (int64_t)img.size(), N = y.size(0), C = y.size(-1);
  TORCH_CHECK(N <= 65535 && C <= INT_MAX, "imgcomp_rate: y is too large: ", y.sizes());
  return symbolize_candidates("imgcomp_rate", "gain_symbolize_seg", "candidate", "image", y, mu, img,
                              [&](const int* im, int* img_dev, int* sym, int* kmax_dev, int* kmax_host) {
                                return ic_gain_symbolize_seg(y.data_ptr<float>(), N, y.numel() / N / C, (int)C,
                                                             g.data_ptr<float>(), mu.data_ptr<float>(), (int)M, im, img_dev,
                                                             sym, kmax_dev, kmax_host, stream_of(y));
                              });
}

Tensor rate_measure_seg_meta(const Tensor& sym, int64_t nseg, const std::optional<Tensor>&, int64_t, const Tensor&, int64_t,
                             at::IntArrayRef, at::IntArrayRef, int64_t steps) {
  TORCH_CHECK(nseg >= 1 && sym.numel() % nseg == 0, "imgcomp_rate: symbols do not make equal segments");
  const int64_t chunks = ic_codec_seg_chunks((int)nseg, sym.numel() / nseg, (int)steps);
  TORCH_CHECK(chunks > 0, "imgcomp_rate: bad symbol count or steps_per_chunk");
  return at::empty({chunks}, sym.options().dtype(at::kInt));
}
std::tuple<Tensor, std::vector<int64_t>> rate_gain_symbolize_seg_meta(const Tensor& y, const Tensor& g, const Tensor& mu,
                                                                      at::IntArrayRef img) {
  check_rate_shapes(y, g, mu, img);
  return {symbols_out(mu), std::vector<int64_t>(img.size(), 0)};
}

// ---------------------------------------------------------------- transcoding in the latent domain (imgcomp_transcode)
// r, mu1 (N, *, C) contiguous, read in place; a (N, C); b (M, C); mu2: the M targets' means back to back, each an image
// of r's size; img: the source of every target
void check_transcode_shapes(const Tensor& r, const Tensor& mu1, const Tensor& a, const Tensor& b, const Tensor& mu2,
                            at::IntArrayRef img) {
  const int64_t M = (int64_t)img.size();
  TORCH_CHECK(r.dim() >= 2 && r.numel() > 0, "imgcomp_transcode: r must be a non-empty (N, *, C) tensor, got ", r.sizes());
  TORCH_CHECK(mu1.sizes() == r.sizes(), "imgcomp_transcode: mu1 ", mu1.sizes(), " must have r's shape ", r.sizes());
  TORCH_CHECK(a.dim() == 2 && a.size(0) == r.size(0) && a.size(1) == r.size(-1), "imgcomp_transcode: the source gains ",
              a.sizes(), " must be (", r.size(0), " sources, ", r.size(-1), ")");
  TORCH_CHECK(M >= 1 && M <= 65535 && b.dim() == 2 && b.size(0) == M && b.size(1) == r.size(-1),
              "imgcomp_transcode: the target gains ", b.sizes(), " must be (", M, " targets, ", r.size(-1), ")");
  TORCH_CHECK(mu2.numel() == M * (r.numel() / r.size(0)), "imgcomp_transcode: mu2 (", mu2.numel(), " values) must hold ",
              M, " images of ", r.numel() / r.size(0), " values");
}

std::tuple<Tensor, std::vector<int64_t>> transcode_requant_seg(const Tensor& r, const Tensor& mu1, const Tensor& a,
                                                               const Tensor& b, const Tensor& mu2, at::IntArrayRef img) {
  const std::pair<const Tensor*, const char*> operands[] = {{&r, "r"}, {&mu1, "mu1"}, {&a, "a"}, {&b, "b"}, {&mu2, "mu2"}};
  for (const auto& [t, what] : operands) check_operand(*t, what);
  check_transcode_shapes(r, mu1, a, b, mu2, img);
  for (const auto& [t, what] : operands) {
    TORCH_CHECK(t->is_contiguous(), "imgcomp_transcode: ", what, " must be contiguous");
    TORCH_CHECK(t->device() == r.device(), "imgcomp_transcode: every operand must be on r's device");
  }
  const int64_t M = (int64_t)img.size(), N = r.size(0), C = r.size(-1);
  TORCH_CHECK(N <= 65535 && C <= INT_MAX, "imgcomp_transcode: r is too large: ", r.sizes());
  return symbolize_candidates("imgcomp_transcode", "requant_seg", "target", "source", r, mu2, img,
                              [&](const int* im, int* img_dev, int* sym, int* kmax_dev, int* kmax_host) {
                                return ic_requant_seg(r.data_ptr<float>(), mu1.data_ptr<float>(), N, r.numel() / N / C,
                                                      (int)C, a.data_ptr<float>(), b.data_ptr<float>(),
                                                      mu2.data_ptr<float>(), (int)M, im, img_dev, sym, kmax_dev, kmax_host,
                                                      stream_of(r));
                              });
}

std::tuple<Tensor, std::vector<int64_t>> transcode_requant_seg_meta(const Tensor& r, const Tensor& mu1, const Tensor& a,
                                                                    const Tensor& b, const Tensor& mu2,
                                                                    at::IntArrayRef img) {
  check_transcode_shapes(r, mu1, a, b, mu2, img);
  return {symbols_out(mu2), std::vector<int64_t>(img.size(), 0)};
}

// ---------------------------------------------------------------- a quality map under a byte budget (imgcomp_alloc)
// bits, sse (N, L, nb) contiguous; img, w: the image and the weight of every candidate; codes: the code of every level
void check_alloc_shapes(const Tensor& bits, const Tensor& sse, at::IntArrayRef img, at::ArrayRef<double> w,
                        at::IntArrayRef codes) {
  const int64_t M = (int64_t)img.size();
  TORCH_CHECK(bits.dim() == 3 && bits.numel() > 0 && bits.size(1) >= 2 && bits.size(1) <= 16,
              "imgcomp_alloc: the tables must be non-empty (N, 2 .. 16 levels, blocks) tensors, got ", bits.sizes());
  TORCH_CHECK(sse.sizes() == bits.sizes(), "imgcomp_alloc: the two tables must share a shape, got ", bits.sizes(), " and ",
              sse.sizes());
  TORCH_CHECK(M >= 1 && M <= 65535 && (int64_t)w.size() == M, "imgcomp_alloc: ", M, " images and ", w.size(),
              " weights do not make 1 .. 65535 candidates");
  TORCH_CHECK((int64_t)codes.size() == bits.size(1), "imgcomp_alloc: ", codes.size(), " codes for ", bits.size(1), " levels");
}

std::tuple<Tensor, Tensor, Tensor> alloc_out(const Tensor& bits, int64_t M) {
  const auto bytes = bits.options().dtype(at::kByte);
  return {at::empty({M, bits.size(2)}, bytes), at::empty({M, bits.size(2)}, bytes),
          at::empty({2, M}, bits.options().dtype(at::kDouble))};
}

std::tuple<Tensor, Tensor, Tensor> alloc_block_allocate(const Tensor& bits, const Tensor& sse, at::IntArrayRef img,
                                                        at::ArrayRef<double> w, at::IntArrayRef codes) {
  check_operand(bits, "bits");
  check_operand(sse, "sse");
  check_alloc_shapes(bits, sse, img, w, codes);
  TORCH_CHECK(bits.is_contiguous() && sse.is_contiguous(), "imgcomp_alloc: the tables must be contiguous");
  TORCH_CHECK(bits.device() == sse.device(), "imgcomp_alloc: the tables must be on one device");
  const int64_t M = (int64_t)img.size(), N = bits.size(0), L = bits.size(1);
  TORCH_CHECK(N <= 65535, "imgcomp_alloc: the tables are too large: ", bits.sizes());
  std::vector<int> im;
  std::vector<float> wf;
  std::vector<unsigned char> lc;
  for (int64_t m = 0; m < M; ++m) {
    TORCH_CHECK_VALUE(img[m] >= 0 && img[m] < N, "imgcomp_alloc: candidate ", m, " names image ", img[m], " of ", N);
    const float v = (float)w[m];
    TORCH_CHECK_VALUE(std::isfinite(v) && v >= 0.0f, "imgcomp_alloc: the weight of candidate ", m, " must be finite and "
                      ">= 0, got ", w[m]);
    im.push_back((int)img[m]);
    wf.push_back(v);
  }
  for (int64_t l = 0; l < L; ++l) {
    TORCH_CHECK_VALUE(codes[l] >= 0 && codes[l] <= 255, "imgcomp_alloc: the code of level ", l, " must be in 0 .. 255, got ",
                      codes[l]);
    lc.push_back((unsigned char)codes[l]);
  }
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(bits.device());
  auto [ranks, out_codes, sums] = alloc_out(bits, M);
  Tensor cand = at::empty({2 * M}, bits.options().dtype(at::kInt));   // the images, then the weights
  check_rc(ic_block_allocate(bits.data_ptr<float>(), sse.data_ptr<float>(), (int)N, (int)L, bits.size(2), (int)M, im.data(),
                             wf.data(), lc.data(), cand.data_ptr<int>(), ranks.data_ptr<uint8_t>(),
                             out_codes.data_ptr<uint8_t>(), sums.data_ptr<double>(), stream_of(bits)),
           "block_allocate");
  return {ranks, out_codes, sums};
}

std::tuple<Tensor, Tensor, Tensor> alloc_block_allocate_meta(const Tensor& bits, const Tensor& sse, at::IntArrayRef img,
                                                             at::ArrayRef<double> w, at::IntArrayRef codes) {
  check_alloc_shapes(bits, sse, img, w, codes);
  return alloc_out(bits, (int64_t)img.size());
}

// y (N, Hm, Wm, C) contiguous, read in place; g (R, C); rank: uint8 (M, ceil(Hm / 2^shift), ceil(Wm / 2^shift)); mu: the
// M candidates' means back to back, each an image of y's size; img: the image of every candidate
void check_alloc_symbolize_shapes(const Tensor& y, const Tensor& g, const Tensor& rank, const Tensor& mu,
                                  at::IntArrayRef img, int64_t shift) {
  const int64_t M = (int64_t)img.size();
  TORCH_CHECK_VALUE(shift >= 0 && shift <= 6, "imgcomp_alloc: a block is 2^shift positions wide, shift in 0 .. 6, got ",
                    shift);
  TORCH_CHECK(y.dim() == 4 && y.numel() > 0, "imgcomp_alloc: y must be a non-empty (N, Hm, Wm, C) tensor, got ", y.sizes());
  TORCH_CHECK(g.dim() == 2 && g.size(1) == y.size(3) && g.size(0) >= 1 && g.size(0) <= 256, "imgcomp_alloc: the gains ",
              g.sizes(), " must be (1 .. 256, C) for y ", y.sizes());
  TORCH_CHECK(M >= 1 && M <= 65535, "imgcomp_alloc: ", M, " candidates (1 .. 65535)");
  TORCH_CHECK(rank.scalar_type() == at::kByte && rank.dim() == 3 && rank.size(0) == M &&
                  rank.size(1) == map_extent(y.size(1), shift) && rank.size(2) == map_extent(y.size(2), shift),
              "imgcomp_alloc: the rank map ", rank.sizes(), " must be uint8 (", M, ", ", map_extent(y.size(1), shift), ", ",
              map_extent(y.size(2), shift), ") for y ", y.sizes(), " at shift ", shift);
  TORCH_CHECK(mu.numel() == M * (y.numel() / y.size(0)), "imgcomp_alloc: mu (", mu.numel(), " values) must hold ", M,
              " images of ", y.numel() / y.size(0), " values");
}

std::tuple<Tensor, std::vector<int64_t>> alloc_block_gain_symbolize_seg(const Tensor& y, const Tensor& g, const Tensor& rank,
                                                                        const Tensor& mu, at::IntArrayRef img,
                                                                        int64_t shift) {
  check_operand(y, "y");
  check_operand(g, "g");
  check_operand(mu, "mu");
  TORCH_CHECK(rank.is_cuda(), "imgcomp: the rank map must be on a ROCm device, got ", rank.device());
  check_alloc_symbolize_shapes(y, g, rank, mu, img, shift);
  TORCH_CHECK(y.is_contiguous() && g.is_contiguous() && rank.is_contiguous() && mu.is_contiguous(),
              "imgcomp_alloc: y, g, the rank map and mu must be contiguous");
  TORCH_CHECK(y.device() == g.device() && y.device() == mu.device() && y.device() == rank.device(),
              "imgcomp_alloc: y, g, the rank map and mu must be on one device");
  const int64_t M = (int64_t)img.size(), N = y.size(0);
  TORCH_CHECK(N <= 65535 && y.numel() / N <= INT_MAX, "imgcomp_alloc: y is too large: ", y.sizes());
  return symbolize_candidates("imgcomp_alloc", "block_gain_symbolize_seg", "candidate", "image", y, mu, img,
                              [&](const int* im, int* img_dev, int* sym, int* kmax_dev, int* kmax_host) {
                                return ic_block_gain_symbolize_seg(y.data_ptr<float>(), (int)N, (int)y.size(1),
                                                                   (int)y.size(2), (int)y.size(3), g.data_ptr<float>(),
                                                                   (int)g.size(0), rank.data_ptr<uint8_t>(), (int)shift,
                                                                   mu.data_ptr<float>(), (int)M, im, img_dev, sym, kmax_dev,
                                                                   kmax_host, stream_of(y));
                              });
}

std::tuple<Tensor, std::vector<int64_t>> alloc_block_gain_symbolize_seg_meta(const Tensor& y, const Tensor& g,
                                                                             const Tensor& rank, const Tensor& mu,
                                                                             at::IntArrayRef img, int64_t shift) {
  check_alloc_symbolize_shapes(y, g, rank, mu, img, shift);
  return {symbols_out(mu), std::vector<int64_t>(img.size(), 0)};
}

// ---------------------------------------------------------------- encode-time latent refinement (imgcomp_refine)
// The latent is (N, *, C) contiguous (channels-last storage); v, m and u are updated in place.  Nothing here copies to
// the host or waits for the stream.  Inference only: no autograd node.
void check_refine_latent(const Tensor& v, const std::optional<Tensor>& m, const std::optional<Tensor>& u,
                         const std::optional<Tensor>& g, const std::optional<Tensor>& mu) {
  TORCH_CHECK(v.dim() >= 2 && v.numel() > 0, "imgcomp_refine: v must be a non-empty (N, *, C) tensor, got ", v.sizes());
  TORCH_CHECK(v.size(0) <= 65535 && v.size(-1) <= INT_MAX, "imgcomp_refine: v is too large: ", v.sizes());
  const std::pair<const std::optional<Tensor>*, const char*> rest[] = {{&m, "m"}, {&u, "u"}, {&g, "g"}, {&mu, "mu"}};
  for (const auto& [t, what] : rest)
    if (t->has_value() && (*t)->defined())
      TORCH_CHECK((*t)->sizes() == v.sizes(), "imgcomp_refine: ", what, " ", (*t)->sizes(), " must have v's shape ",
                  v.sizes());
  if (g.has_value() && g->defined())
    TORCH_CHECK(m.has_value() && m->defined() && u.has_value() && u->defined(),
                "imgcomp_refine: a step (g given) needs the moments m and u");
}

void check_refine_step(const std::optional<Tensor>& g, double lr, double c1, double c2) {
  if (!g.has_value() || !g->defined()) return;
  TORCH_CHECK_VALUE(std::isfinite(lr) && lr > 0.0, "imgcomp_refine: lr must be finite and positive, got ", lr);
  TORCH_CHECK_VALUE(std::isfinite(c1) && c1 >= 1.0 && std::isfinite(c2) && c2 >= 1.0,
                    "imgcomp_refine: the bias corrections 1 / (1 - beta^t) are finite and >= 1, got ", c1, " and ", c2);
}

std::tuple<Tensor, Tensor> refine_update(Tensor& v, const std::optional<Tensor>& m, const std::optional<Tensor>& u,
                                         const std::optional<Tensor>& g, const std::optional<Tensor>& mu, double lr,
                                         double c1, double c2) {
  check_refine_latent(v, m, u, g, mu);
  check_refine_step(g, lr, c1, c2);
  check_operand(v, "v");
  TORCH_CHECK(v.is_contiguous(), "imgcomp_refine: v must be contiguous");
  const std::pair<const std::optional<Tensor>*, const char*> rest[] = {{&m, "m"}, {&u, "u"}, {&g, "g"}, {&mu, "mu"}};
  for (const auto& [t, what] : rest)
    if (t->has_value() && (*t)->defined()) {
      check_operand(**t, what);
      TORCH_CHECK((*t)->is_contiguous() && (*t)->device() == v.device(), "imgcomp_refine: ", what,
                  " must be contiguous and on v's device");
    }
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(v.device());
  Tensor sym = symbols_out(v);
  Tensor y_hat = at::empty(v.sizes(), v.options());
  const int64_t N = v.size(0), C = v.size(-1);
  check_rc(ic_refine_update(v.data_ptr<float>(), opt_ptr(m), opt_ptr(u), opt_ptr(g), opt_ptr(mu), N, v.numel() / N / C,
                            (int)C, (float)lr, (float)c1, (float)c2, sym.data_ptr<int>(), y_hat.data_ptr<float>(),
                            stream_of(v)),
           "refine_update");
  return {sym, y_hat};
}

void check_refine_images(const Tensor& x, const Tensor& x_hat, const Tensor& w) {
  TORCH_CHECK(x.dim() >= 2 && x.numel() > 0 && x.size(0) <= 65535, "imgcomp_refine: x must be a non-empty (N, *) batch of "
              "at most 65535 images, got ", x.sizes());
  TORCH_CHECK(x_hat.sizes() == x.sizes(), "imgcomp_refine: x_hat ", x_hat.sizes(), " must have x's shape ", x.sizes());
  TORCH_CHECK(w.dim() == 1 && w.size(0) == x.size(0) && w.scalar_type() == at::kDouble,
              "imgcomp_refine: w must hold one float64 weight per image");
}

Tensor refine_dist_grad(const Tensor& x, const Tensor& x_hat, const Tensor& w) {
  check_refine_images(x, x_hat, w);
  check_operand(x, "x");
  check_operand(x_hat, "x_hat");
  TORCH_CHECK(w.is_cuda() && w.is_contiguous() && x.is_contiguous() && x_hat.is_contiguous() &&
                  x.device() == x_hat.device() && x.device() == w.device(),
              "imgcomp_refine: x, x_hat and w must be contiguous on one ROCm device");
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(x.device());
  Tensor gx = at::empty(x.sizes(), x.options());
  check_rc(ic_refine_dist_grad(x.data_ptr<float>(), x_hat.data_ptr<float>(), w.data_ptr<double>(), (int)x.size(0),
                               x.numel() / x.size(0), gx.data_ptr<float>(), stream_of(x)),
           "refine_dist_grad");
  return gx;
}

void check_refine_maps(const Tensor& bits, const Tensor& sse, const Tensor& w) {
  TORCH_CHECK(bits.dim() >= 2 && bits.numel() > 0 && bits.size(0) <= 65535,
              "imgcomp_refine: bits must be a non-empty (N, *) map of at most 65535 images, got ", bits.sizes());
  TORCH_CHECK(sse.sizes() == bits.sizes(), "imgcomp_refine: the maps must share a shape, got ", bits.sizes(), " and ",
              sse.sizes());
  TORCH_CHECK(w.dim() == 1 && w.size(0) == bits.size(0) && w.scalar_type() == at::kDouble,
              "imgcomp_refine: w must hold one float64 weight per image");
}

Tensor refine_objective(const Tensor& bits, const Tensor& sse, const Tensor& w) {
  check_refine_maps(bits, sse, w);
  check_operand(bits, "bits");
  check_operand(sse, "sse");
  TORCH_CHECK(w.is_cuda() && w.is_contiguous() && bits.is_contiguous() && sse.is_contiguous() &&
                  bits.device() == sse.device() && bits.device() == w.device(),
              "imgcomp_refine: bits, sse and w must be contiguous on one ROCm device");
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(bits.device());
  const int64_t N = bits.size(0);
  Tensor out = at::empty({3, N}, w.options());
  check_rc(ic_refine_objective(bits.data_ptr<float>(), sse.data_ptr<float>(), w.data_ptr<double>(), (int)N,
                               bits.numel() / N, out.data_ptr<double>(), stream_of(bits)),
           "refine_objective");
  return out;
}

void check_refine_keep(const Tensor& sym, const Tensor& best_sym, const Tensor& obj, const Tensor& best,
                       const Tensor& best_step, int64_t step) {
  TORCH_CHECK(obj.dim() == 2 && obj.size(0) == 3 && obj.size(1) >= 1 && obj.size(1) <= 65535 &&
                  obj.scalar_type() == at::kDouble,
              "imgcomp_refine: obj must be float64 (3, N), got ", obj.sizes());
  const int64_t N = obj.size(1);
  TORCH_CHECK(best.sizes() == obj.sizes() && best.scalar_type() == at::kDouble,
              "imgcomp_refine: best must be float64 (3, N) like obj, got ", best.sizes());
  TORCH_CHECK(best_step.dim() == 1 && best_step.size(0) == N && best_step.scalar_type() == at::kInt,
              "imgcomp_refine: best_step must be int32 (N)");
  TORCH_CHECK(sym.scalar_type() == at::kInt && best_sym.scalar_type() == at::kInt && sym.numel() > 0 &&
                  sym.numel() == best_sym.numel() && sym.numel() % N == 0,
              "imgcomp_refine: sym and best_sym must be int32 and hold the ", N, " images' symbols back to back");
  TORCH_CHECK_VALUE(step >= 0 && step <= INT_MAX, "imgcomp_refine: step must be >= 0, got ", step);
}

void refine_keep(const Tensor& sym, Tensor& best_sym, const Tensor& obj, Tensor& best, Tensor& best_step, int64_t step) {
  check_refine_keep(sym, best_sym, obj, best, best_step, step);
  for (const Tensor* t : std::initializer_list<const Tensor*>{&sym, &best_sym, &obj, &best, &best_step})
    TORCH_CHECK(t->is_cuda() && t->is_contiguous() && t->device() == sym.device(),
                "imgcomp_refine: every operand of keep must be contiguous on one ROCm device");
  TORCH_CHECK(sym.data_ptr() != best_sym.data_ptr(), "imgcomp_refine: sym and best_sym must be two buffers");
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(sym.device());
  const int64_t N = obj.size(1);
  for (int mode = 0; mode < 2; ++mode)   // the symbols first, then the scalars the comparison reads
    check_rc(ic_refine_keep(sym.data_ptr<int>(), best_sym.data_ptr<int>(), obj.data_ptr<double>(), best.data_ptr<double>(),
                            best_step.data_ptr<int>(), (int)step, (int)N, sym.numel() / N, mode, stream_of(sym)),
             "refine_keep");
}

Tensor refine_kmax(const Tensor& sym, int64_t nseg) {
  TORCH_CHECK(nseg >= 1 && nseg <= 65535 && sym.scalar_type() == at::kInt && sym.numel() > 0 && sym.numel() % nseg == 0,
              "imgcomp_refine: sym must be int32 and make ", nseg, " equal segments");
  check_codec(sym, at::kInt, "sym");
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(sym.device());
  Tensor kmax = at::empty({nseg}, sym.options());
  check_rc(ic_refine_kmax(sym.data_ptr<int>(), (int)nseg, sym.numel() / nseg, kmax.data_ptr<int>(), stream_of(sym)),
           "refine_kmax");
  return kmax;
}

std::tuple<Tensor, Tensor> refine_update_meta(Tensor& v, const std::optional<Tensor>& m, const std::optional<Tensor>& u,
                                              const std::optional<Tensor>& g, const std::optional<Tensor>& mu, double lr,
                                              double c1, double c2) {
  check_refine_latent(v, m, u, g, mu);
  check_refine_step(g, lr, c1, c2);
  return {symbols_out(v), at::empty(v.sizes(), v.options())};
}
Tensor refine_dist_grad_meta(const Tensor& x, const Tensor& x_hat, const Tensor& w) {
  check_refine_images(x, x_hat, w);
  return at::empty(x.sizes(), x.options());
}
Tensor refine_objective_meta(const Tensor& bits, const Tensor& sse, const Tensor& w) {
  check_refine_maps(bits, sse, w);
  return at::empty({3, bits.size(0)}, w.options());
}
void refine_keep_meta(const Tensor& sym, Tensor& best_sym, const Tensor& obj, Tensor& best, Tensor& best_step,
                      int64_t step) {
  check_refine_keep(sym, best_sym, obj, best, best_step, step);
}
Tensor refine_kmax_meta(const Tensor& sym, int64_t nseg) {
  TORCH_CHECK(nseg >= 1 && nseg <= 65535 && sym.scalar_type() == at::kInt && sym.numel() > 0 && sym.numel() % nseg == 0,
              "imgcomp_refine: sym must be int32 and make ", nseg, " equal segments");
  return at::empty({nseg}, sym.options());
}

// ---------------------------------------------------------------- decoding a window of a latent (imgcomp_window)
// windows: nine integers per window, ic_window's fields in their order (base, table, hy, wy, K, r0, c0, k0, k1);
// spans: (begin, end) in 16-bit words of `packed` per (window, chunk).  The shapes are checked here, every
// descriptor by the C entry point, before anything is launched.
constexpr int64_t WINDOW_FIELDS = 9;

int64_t check_window_shapes(const Tensor& packed, at::IntArrayRef windows, int64_t rh, int64_t rw, at::IntArrayRef spans,
                            const std::optional<Tensor>& rows, const std::optional<Tensor>& mu, int64_t C,
                            const Tensor& pool, int64_t nrows, int64_t steps) {
  TORCH_CHECK(packed.scalar_type() == at::kByte && packed.dim() == 1 && packed.numel() > 0,
              "imgcomp_window: packed must be a non-empty 1-D uint8 buffer");
  TORCH_CHECK(pool.scalar_type() == at::kInt && pool.numel() > 0, "imgcomp_window: the table pool must be int32");
  const int64_t nwin = (int64_t)windows.size() / WINDOW_FIELDS;
  TORCH_CHECK(nwin >= 1 && nwin <= 65535 && (int64_t)windows.size() == nwin * WINDOW_FIELDS,
              "imgcomp_window: windows holds ", WINDOW_FIELDS, " integers for each of 1 .. 65535 windows, got ",
              windows.size());
  TORCH_CHECK(spans.size() >= 2 && spans.size() % 2 == 0 && spans.size() / 2 <= (size_t)INT_MAX,
              "imgcomp_window: spans holds (begin, end) per block, got ", spans.size(), " integers");
  TORCH_CHECK(rh >= 1 && rw >= 1 && rh <= INT_MAX && rw <= INT_MAX && C >= 1 && C <= INT_MAX && nrows >= 1 &&
                  nrows <= INT_MAX && rh * rw <= INT_MAX / C,
              "imgcomp_window: a window is rh x rw positions of C channels, below 2^31 values");
  TORCH_CHECK(steps >= 1 && steps <= IC_CODEC_MAXR, "imgcomp_window: steps_per_chunk in [1, ", IC_CODEC_MAXR, "]");
  for (int64_t k = 0; k < nwin; ++k)
    for (int64_t f = 2; f < WINDOW_FIELDS; ++f)
      TORCH_CHECK(windows[k * WINDOW_FIELDS + f] >= INT_MIN && windows[k * WINDOW_FIELDS + f] <= INT_MAX,
                  "imgcomp_window: field ", f, " of window ", k, " is not an int");
  const bool hr = rows.has_value() && rows->defined(), hm = mu.has_value() && mu->defined();
  TORCH_CHECK(!hr || rows->scalar_type() == at::kByte, "imgcomp_window: rows must be uint8");
  TORCH_CHECK(!hm || mu->scalar_type() == at::kFloat, "imgcomp_window: mu must be float32");
  TORCH_CHECK(!hr || !hm || rows->numel() == mu->numel(), "imgcomp_window: rows and mu must hold one value per symbol");
  return nwin;
}

Tensor window_decode(const Tensor& packed, at::IntArrayRef windows, int64_t rh, int64_t rw, at::IntArrayRef spans,
                     const std::optional<Tensor>& rows, const std::optional<Tensor>& mu, int64_t C, const Tensor& pool,
                     int64_t nrows, int64_t steps) {
  const int64_t nwin = check_window_shapes(packed, windows, rh, rw, spans, rows, mu, C, pool, nrows, steps);
  check_codec(packed, at::kByte, "packed");
  check_codec(pool, at::kInt, "table pool");
  const bool hr = rows.has_value() && rows->defined(), hm = mu.has_value() && mu->defined();
  if (hr) check_codec(*rows, at::kByte, "rows");
  if (hm) {
    check_dense(*mu, "mu");
    TORCH_CHECK(mu->is_contiguous(), "imgcomp_window: mu must be contiguous");
  }
  for (const Tensor* t : {&pool, hr ? &*rows : &packed, hm ? &*mu : &packed})
    TORCH_CHECK(t->device() == packed.device(), "imgcomp_window: every operand must be on packed's device");
  TORCH_CHECK(((uintptr_t)packed.data_ptr() & 1) == 0, "imgcomp_window: packed buffer must be 2-byte aligned");
  std::vector<ic_window> win((size_t)nwin);
  for (int64_t k = 0; k < nwin; ++k) {
    const int64_t* f = windows.data() + k * WINDOW_FIELDS;
    win[(size_t)k] = ic_window{f[0], f[1], (int)f[2], (int)f[3], (int)f[4], (int)f[5], (int)f[6], (int)f[7], (int)f[8]};
  }
  const std::vector<long long> sp(spans.begin(), spans.end());
  const int64_t nblocks = (int64_t)sp.size() / 2;
  // with neither rows nor a mean nothing is indexed by a symbol's number: no bound on the segments' ends
  const int64_t nsym = hr ? rows->numel() : (hm ? mu->numel() : INT64_MAX);
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(packed.device());
  const size_t wsb = ic_codec_window_ws((int)nwin, nblocks);
  Tensor ws = at::empty({(int64_t)std::max<size_t>(wsb, 8) / 8 + 1}, packed.options().dtype(at::kLong));
  Tensor out = at::empty({nwin, rh, rw, C}, packed.options().dtype(at::kFloat));
  check_rc(ic_codec_decode_window(packed.data_ptr(), (size_t)packed.numel(), win.data(), (int)nwin, (int)rh, (int)rw,
                                  sp.data(), nblocks, hr ? rows->data_ptr<unsigned char>() : nullptr,
                                  hm ? mu->data_ptr<float>() : nullptr, nsym, (int)C,
                                  (const unsigned int*)pool.data_ptr<int>(), (size_t)pool.numel(), (int)nrows, (int)steps,
                                  ws.data_ptr(), (size_t)ws.numel() * 8, out.data_ptr<float>(), stream_of(packed)),
           "codec_decode_window");
  return out;
}

void check_crop_at(const Tensor& x, int64_t top, int64_t left, int64_t h, int64_t w) {
  TORCH_CHECK(x.dim() == 4 && x.numel() > 0 && h >= 1 && w >= 1 && top >= 0 && left >= 0 && h <= x.size(2) &&
                  w <= x.size(3) && top <= x.size(2) - h && left <= x.size(3) - w,
              "imgcomp_window: crop_clamp_at takes (N, C, H, W) and a rectangle inside H x W, got ", x.sizes(), " -> ", h,
              " x ", w, " at (", top, ", ", left, ")");
}

Tensor window_crop_clamp_at(const Tensor& x, int64_t top, int64_t left, int64_t h, int64_t w) {
  check_operand(x, "x");
  check_crop_at(x, top, left, h, w);
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(x.device());
  Tensor y = at::empty({x.size(0), x.size(1), h, w}, x.options().memory_format(at::MemoryFormat::Contiguous));
  const ic_act ax = act_of(x);
  check_rc(ic_crop_clamp_at(&ax, (int)top, (int)left, (int)h, (int)w, y.data_ptr<float>(), stream_of(x)), "crop_clamp_at");
  return y;
}

Tensor window_decode_meta(const Tensor& packed, at::IntArrayRef windows, int64_t rh, int64_t rw, at::IntArrayRef spans,
                          const std::optional<Tensor>& rows, const std::optional<Tensor>& mu, int64_t C, const Tensor& pool,
                          int64_t nrows, int64_t steps) {
  const int64_t nwin = check_window_shapes(packed, windows, rh, rw, spans, rows, mu, C, pool, nrows, steps);
  return at::empty({nwin, rh, rw, C}, packed.options().dtype(at::kFloat));
}
Tensor window_crop_clamp_at_meta(const Tensor& x, int64_t top, int64_t left, int64_t h, int64_t w) {
  check_crop_at(x, top, left, h, w);
  return at::empty({x.size(0), x.size(1), h, w}, x.options().memory_format(at::MemoryFormat::Contiguous));
}

// ---------------------------------------------------------------- layered per-image streams (imgcomp_layer)
// The dense side is (N, P, C), channel fastest; order holds N rows of C channel numbers and G layers share them.
// Shapes and counts are checked here (and by the Meta kernels); every entry of order, seg and nlayers by the C entry
// points, before anything is launched.
void check_layer_counts(int64_t N, int64_t P, int64_t C, int64_t G, int64_t order_size) {
  TORCH_CHECK(N >= 1 && N <= INT_MAX && P >= 1 && C >= 1 && C <= INT_MAX && P <= (INT64_MAX / 8) / C / N,
              "imgcomp_layer: (N, P, C) = (", N, ", ", P, ", ", C, ") is empty or too large");
  TORCH_CHECK(G >= 1 && G <= C && C % G == 0, "imgcomp_layer: ", G, " layers do not divide ", C, " channels");
  TORCH_CHECK(order_size == N * C, "imgcomp_layer: order holds ", order_size, " entries, not N C = ", N * C);
}

void check_layer_dense(const Tensor& t, const char* what) {
  TORCH_CHECK(t.dim() == 3 && t.is_contiguous() && t.numel() > 0, "imgcomp_layer: ", what,
              " must be a non-empty contiguous (N, P, C) tensor, got ", t.sizes());
}

std::vector<int> layer_ints(at::IntArrayRef v, const char* what) {
  std::vector<int> out(v.size());
  for (size_t i = 0; i < v.size(); ++i) {
    TORCH_CHECK(v[i] >= INT_MIN && v[i] <= INT_MAX, "imgcomp_layer: entry ", i, " of ", what, " is not an int");
    out[i] = (int)v[i];
  }
  return out;
}

int64_t check_layer_gather(const Tensor& src, int64_t G, at::IntArrayRef order, at::IntArrayRef seg) {
  check_layer_dense(src, "src");
  const auto ty = src.scalar_type();
  TORCH_CHECK(ty == at::kByte || ty == at::kInt || ty == at::kFloat, "imgcomp_layer: src must be uint8, int32 or float32, got ",
              ty);
  check_layer_counts(src.size(0), src.size(1), src.size(2), G, (int64_t)order.size());
  const int64_t nseg = (int64_t)seg.size() / 2;
  TORCH_CHECK(nseg >= 1 && nseg <= 65535 && (int64_t)seg.size() == 2 * nseg,
              "imgcomp_layer: seg holds (image, layer) for each of 1 .. 65535 segments, got ", seg.size(), " integers");
  return nseg;
}

void check_layer_scatter(const Tensor& q, const std::optional<Tensor>& mu, int64_t N, int64_t P, int64_t C, int64_t G,
                         at::IntArrayRef order, at::IntArrayRef nlayers) {
  check_layer_counts(N, P, C, G, (int64_t)order.size());
  TORCH_CHECK((int64_t)nlayers.size() == N, "imgcomp_layer: nlayers holds ", nlayers.size(), " entries, not N = ", N);
  int64_t sum = 0;
  for (int64_t v : nlayers) {
    TORCH_CHECK(v >= 0 && v <= G, "imgcomp_layer: an image brings 0 .. ", G, " layers, got ", v);
    sum += v;
  }
  TORCH_CHECK(q.scalar_type() == at::kFloat && q.numel() == sum * P * (C / G), "imgcomp_layer: q must hold the ", sum,
              " layers present as float32, ", sum * P * (C / G), " values, got ", q.numel(), " of ", q.scalar_type());
  if (mu.has_value() && mu->defined()) {
    check_layer_dense(*mu, "mu");
    TORCH_CHECK(mu->scalar_type() == at::kFloat && mu->size(0) == N && mu->size(1) == P && mu->size(2) == C,
                "imgcomp_layer: mu must be float32 (", N, ", ", P, ", ", C, "), got ", mu->sizes());
  }
}

Tensor layer_energy(const Tensor& sym) {
  check_layer_dense(sym, "sym");
  check_codec(sym, at::kInt, "sym");
  const int64_t N = sym.size(0), P = sym.size(1), C = sym.size(2);
  check_layer_counts(N, P, C, 1, N * C);
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(sym.device());
  Tensor energy = at::empty({N, C}, sym.options().dtype(at::kLong));
  check_rc(ic_layer_energy(sym.data_ptr<int>(), (int)N, P, (int)C, (unsigned long long*)energy.data_ptr<int64_t>(),
                           stream_of(sym)),
           "layer_energy");
  return energy;
}

Tensor layer_gather(const Tensor& src, int64_t G, at::IntArrayRef order, at::IntArrayRef seg) {
  const int64_t nseg = check_layer_gather(src, G, order, seg);
  TORCH_CHECK(src.is_cuda(), "imgcomp_layer: src must be on a ROCm device, got ", src.device());
  const int64_t N = src.size(0), P = src.size(1), C = src.size(2);
  const std::vector<int> ord = layer_ints(order, "order"), sg = layer_ints(seg, "seg");
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(src.device());
  Tensor dst = at::empty({nseg * P * (C / G)}, src.options());
  Tensor ints = at::empty({N * C + 4 * nseg + N + 1}, src.options().dtype(at::kInt));
  int* dev = ints.data_ptr<int>();
  check_rc(ic_layer_gather(src.data_ptr(), (int)src.element_size(), (int)N, P, (int)C, (int)G, ord.data(), dev, sg.data(),
                           dev + N * C, (int)nseg, dst.data_ptr(), stream_of(src)),
           "layer_gather");
  return dst;
}

Tensor layer_scatter(const Tensor& q, const std::optional<Tensor>& mu, int64_t N, int64_t P, int64_t C, int64_t G,
                     at::IntArrayRef order, at::IntArrayRef nlayers) {
  check_layer_scatter(q, mu, N, P, C, G, order, nlayers);
  const bool hm = mu.has_value() && mu->defined();
  TORCH_CHECK(q.is_cuda() && q.is_contiguous(), "imgcomp_layer: q must be contiguous on a ROCm device, got ", q.device());
  TORCH_CHECK(!hm || mu->device() == q.device(), "imgcomp_layer: mu must be on q's device");
  const std::vector<int> ord = layer_ints(order, "order"), nl = layer_ints(nlayers, "nlayers");
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(q.device());
  Tensor y_hat = at::empty({N, P, C}, q.options());
  Tensor ints = at::empty({N * C + 2 * N}, q.options().dtype(at::kInt));
  int* dev = ints.data_ptr<int>();
  check_rc(ic_layer_scatter(q.numel() ? q.data_ptr<float>() : nullptr, hm ? mu->data_ptr<float>() : nullptr, (int)N, P,
                            (int)C, (int)G, ord.data(), dev, nl.data(), dev + N * C, y_hat.data_ptr<float>(),
                            stream_of(q)),
           "layer_scatter");
  return y_hat;
}

Tensor layer_energy_meta(const Tensor& sym) {
  check_layer_dense(sym, "sym");
  return at::empty({sym.size(0), sym.size(2)}, sym.options().dtype(at::kLong));
}
Tensor layer_gather_meta(const Tensor& src, int64_t G, at::IntArrayRef order, at::IntArrayRef seg) {
  const int64_t nseg = check_layer_gather(src, G, order, seg);
  return at::empty({nseg * src.size(1) * (src.size(2) / G)}, src.options());
}
Tensor layer_scatter_meta(const Tensor& q, const std::optional<Tensor>& mu, int64_t N, int64_t P, int64_t C, int64_t G,
                          at::IntArrayRef order, at::IntArrayRef nlayers) {
  check_layer_scatter(q, mu, N, P, C, G, order, nlayers);
  return at::empty({N, P, C}, q.options());
}

}  // namespace

TORCH_LIBRARY(imgcomp, m) {
  m.def("conv2d_fwd(Tensor x, Tensor weight, Tensor? bias, int stride, int padding, int act, int math) -> Tensor");
  m.def("conv2d_fwd_ws(Tensor x, Tensor weight, Tensor? bias, int stride, int padding, int act, int math, "
        "Tensor(a!) ws) -> Tensor");
  m.def("conv2d_dgrad(Tensor dy, Tensor weight, Tensor x, int stride, int padding, int math) -> Tensor");
  m.def("conv2d_wgrad(Tensor x, Tensor dy, Tensor weight, int stride, int padding, bool bias, int math) -> "
        "(Tensor, Tensor)");
  m.def("conv_transpose2d_fwd(Tensor x, Tensor weight, Tensor? bias, int stride, int padding, int output_padding, "
        "int act, int math) -> Tensor");
  m.def("conv_transpose2d_fwd_ws(Tensor x, Tensor weight, Tensor? bias, int stride, int padding, "
        "int output_padding, int act, int math, Tensor(a!) ws) -> Tensor");
  m.def("conv_transpose2d_dgrad(Tensor dy, Tensor weight, Tensor x, int stride, int padding, int math) -> Tensor");
  m.def("conv_transpose2d_wgrad(Tensor x, Tensor dy, Tensor weight, int stride, int padding, bool bias, int math) -> "
        "(Tensor, Tensor)");
  m.def("gdn_fwd(Tensor x, Tensor gamma, Tensor beta, bool inverse, int math) -> (Tensor, Tensor)");
  m.def("gdn_bwd(Tensor x, Tensor norm, Tensor dy, Tensor gamma, bool inverse, int math) -> (Tensor, Tensor, Tensor)");
  m.def("gdn_bwd_sum(Tensor x, Tensor norm, Tensor dy, Tensor gamma, bool inverse, int math) -> "
        "(Tensor, Tensor, Tensor, Tensor)");
  m.def("gdn_fwd_xb(Tensor x, Tensor gamma, Tensor beta, bool inverse, int math) -> (Tensor, Tensor, Tensor)");
  m.def("gdn_bwd_sum_xb(Tensor x, Tensor norm, Tensor dy, Tensor gamma, bool inverse, int math) -> "
        "(Tensor, Tensor, Tensor, Tensor, Tensor)");
  m.def("gdn_fwd_rn(Tensor x, Tensor gamma, Tensor beta, bool inverse, int math, bool xb) -> (Tensor, Tensor)");
  m.def("gdn_bwd_sum_rn(Tensor x, Tensor beta, Tensor dy, Tensor gamma, bool inverse, int math, bool xb) -> "
        "(Tensor, Tensor, Tensor, Tensor, Tensor)");
  m.def("conv2d_fwd_xb(Tensor x, Tensor xb, Tensor weight, Tensor? bias, int stride, int padding, int act, "
        "int math) -> Tensor");
  m.def("conv_transpose2d_dgrad_xb(Tensor dy, Tensor dyb, Tensor weight, Tensor x, int stride, int padding, "
        "int math) -> Tensor");
  m.def("conv2d_dgrad_xb(Tensor dy, Tensor dyb, Tensor weight, Tensor x, int stride, int padding, int math) -> Tensor");
  m.def("conv2d_wgrad_xb(Tensor x, Tensor xb, Tensor dy, Tensor dyb, Tensor weight, int stride, int padding, "
        "bool bias, int math) -> (Tensor, Tensor)");
  m.def("conv_transpose2d_wgrad_xb(Tensor x, Tensor xb, Tensor dy, Tensor dyb, Tensor weight, int stride, "
        "int padding, bool bias, int math) -> (Tensor, Tensor)");
  m.def("conv_transpose2d_fwd_xb(Tensor x, Tensor xb, Tensor weight, Tensor? bias, int stride, int padding, "
        "int output_padding, int act, int math) -> Tensor");
  m.def("nonneg_fwd(Tensor p, float bound, float pedestal) -> Tensor");
  m.def("nonneg_bwd(Tensor p, Tensor grad, float bound) -> Tensor");
  m.def("nonneg_multi_fwd(Tensor[] p, float[] bound, float[] pedestal) -> Tensor[]");
  m.def("nonneg_multi_bwd(Tensor[] p, Tensor[] grad, float[] bound) -> Tensor[]");
  m.def("bound_fwd(Tensor x, float bound, bool upper) -> Tensor");
  m.def("bound_bwd(Tensor x, Tensor grad, float bound, bool upper) -> Tensor");
  m.def("relu_fwd(Tensor x) -> Tensor");
  m.def("relu_bwd(Tensor y, Tensor grad) -> Tensor");
  m.def("abs_fwd(Tensor x) -> Tensor");
  m.def("abs_bwd(Tensor x, Tensor grad) -> Tensor");
  m.def("exp_clamp_fwd(Tensor v, float lo, float hi) -> (Tensor, Tensor)");
  m.def("exp_clamp_bwd(Tensor e, Tensor grad, float lo, float hi) -> Tensor");
  m.def("ce_loss_fwd(Tensor p) -> Tensor");
  m.def("ce_loss_bwd(Tensor p, Tensor grad) -> Tensor");
  m.def("mse_fwd(Tensor input, Tensor target) -> Tensor");
  m.def("mse_bwd(Tensor input, Tensor target, Tensor grad, bool need_input, bool need_target) -> (Tensor, Tensor)");
  m.def("sqdiff_fwd(Tensor input, Tensor target) -> Tensor");
  m.def("sqdiff_bwd(Tensor input, Tensor target, Tensor grad, bool need_input, bool need_target) -> (Tensor, Tensor)");
  m.def("factorized_fwd(Tensor z, int channels, Tensor[] params, int mode, Tensor? u, int seed, int offset) -> "
        "(Tensor, Tensor)");
  m.def("factorized_bwd(Tensor q, int channels, Tensor[] params, Tensor? dq, Tensor? dp) -> (Tensor, Tensor[])");
  m.def("factorized_net_fwd(Tensor z, int channels, int[] dims, float bin, Tensor[] params, int mode, Tensor? u, "
        "int seed, int offset) -> (Tensor, Tensor)");
  m.def("factorized_net_bwd(Tensor q, int channels, int[] dims, float bin, Tensor[] params, Tensor? dq, Tensor? dp) -> "
        "(Tensor, Tensor[])");
  m.def("quantize(Tensor y, int mode, Tensor? u, int seed, int offset, float bin) -> Tensor");
  m.def("conditional_fwd(Tensor y, Tensor scale, Tensor? mean, int kind, int mode, Tensor? u, int seed, int offset, "
        "float bin) -> (Tensor, Tensor)");
  m.def("conditional_bwd(Tensor q, Tensor scale, Tensor? mean, int kind, float bin, Tensor? dq, Tensor? dp, "
        "bool need_y, bool need_scale, bool need_mean) -> (Tensor, Tensor, Tensor)");
  m.def("philox_advance(Tensor(a!) state, int n) -> ()");
  m.def("msssim_fwd(Tensor img1, Tensor img2, int levels, int filter_size, float filter_sigma, float max_val, "
        "bool log_scale, int single, float k1, float k2, float eps, float[] weights) -> (Tensor, Tensor)");
  m.def("msssim_bwd(Tensor grad, Tensor state, int[] shape, int levels, int filter_size, float filter_sigma, "
        "float max_val, bool log_scale, int single, float k1, float k2, float eps, float[] weights, bool need_img1, "
        "bool need_img2) -> (Tensor, Tensor)");
}

// The conv / GDN launchers are registered for CPU tensors as well, which their operand checks refuse by name
// ("x must be on a ROCm device"): there is no CPU path, and the launcher says so itself.
static void impl_conv_gdn(torch::Library& m) {
  m.impl("conv2d_fwd", conv2d_fwd);
  m.impl("conv2d_fwd_ws", conv2d_fwd_ws);
  m.impl("conv_transpose2d_fwd_ws", conv_transpose2d_fwd_ws);
  m.impl("conv2d_dgrad", conv2d_dgrad);
  m.impl("conv2d_wgrad", conv2d_wgrad);
  m.impl("conv_transpose2d_fwd", conv_transpose2d_fwd);
  m.impl("conv_transpose2d_dgrad", conv_transpose2d_dgrad);
  m.impl("conv_transpose2d_wgrad", conv_transpose2d_wgrad);
  m.impl("gdn_fwd", gdn_fwd);
  m.impl("gdn_bwd", gdn_bwd);
  m.impl("gdn_bwd_sum", gdn_bwd_sum);
  m.impl("gdn_fwd_xb", gdn_fwd_xb);
  m.impl("gdn_bwd_sum_xb", gdn_bwd_sum_xb);
  m.impl("gdn_fwd_rn", gdn_fwd_rn);
  m.impl("gdn_bwd_sum_rn", gdn_bwd_sum_rn);
  m.impl("conv2d_fwd_xb", conv2d_fwd_xb);
  m.impl("conv_transpose2d_dgrad_xb", conv_transpose2d_dgrad_xb);
  m.impl("conv2d_dgrad_xb", conv2d_dgrad_xb);
  m.impl("conv2d_wgrad_xb", conv2d_wgrad_xb);
  m.impl("conv_transpose2d_wgrad_xb", conv_transpose2d_wgrad_xb);
  m.impl("conv_transpose2d_fwd_xb", conv_transpose2d_fwd_xb);
}

TORCH_LIBRARY_IMPL(imgcomp, CPU, m) { impl_conv_gdn(m); }

TORCH_LIBRARY_IMPL(imgcomp, CUDA, m) {  // the CUDA dispatch key is PyTorch-ROCm's HIP device key
  impl_conv_gdn(m);
  m.impl("nonneg_fwd", nonneg_fwd);
  m.impl("nonneg_bwd", nonneg_bwd);
  m.impl("nonneg_multi_fwd", nonneg_multi_fwd);
  m.impl("nonneg_multi_bwd", nonneg_multi_bwd);
  m.impl("bound_fwd", bound_fwd);
  m.impl("bound_bwd", bound_bwd);
  m.impl("relu_fwd", relu_fwd);
  m.impl("relu_bwd", relu_bwd);
  m.impl("abs_fwd", abs_fwd);
  m.impl("abs_bwd", abs_bwd);
  m.impl("exp_clamp_fwd", exp_clamp_fwd);
  m.impl("exp_clamp_bwd", exp_clamp_bwd);
  m.impl("ce_loss_fwd", ce_loss_fwd);
  m.impl("ce_loss_bwd", ce_loss_bwd);
  m.impl("mse_fwd", mse_fwd);
  m.impl("mse_bwd", mse_bwd);
  m.impl("sqdiff_fwd", sqdiff_fwd);
  m.impl("sqdiff_bwd", sqdiff_bwd);
  m.impl("factorized_fwd", factorized_fwd);
  m.impl("factorized_bwd", factorized_bwd);
  m.impl("factorized_net_fwd", factorized_net_fwd);
  m.impl("factorized_net_bwd", factorized_net_bwd);
  m.impl("quantize", quantize);
  m.impl("conditional_fwd", conditional_fwd);
  m.impl("conditional_bwd", conditional_bwd);
  m.impl("philox_advance", philox_advance);
  m.impl("msssim_fwd", msssim_fwd);
  m.impl("msssim_bwd", msssim_bwd);
}

TORCH_LIBRARY_IMPL(imgcomp, Meta, m) {
  m.impl("conv2d_fwd", conv2d_fwd_meta);
  m.impl("conv2d_fwd_ws", conv2d_fwd_ws_meta);
  m.impl("conv_transpose2d_fwd_ws", conv_transpose2d_fwd_ws_meta);
  m.impl("conv2d_dgrad", conv_dgrad_meta<true>);
  m.impl("conv2d_wgrad", conv_wgrad_meta<false>);
  m.impl("conv_transpose2d_fwd", conv_transpose2d_fwd_meta);
  m.impl("conv_transpose2d_dgrad", conv_dgrad_meta<false>);
  m.impl("conv_transpose2d_wgrad", conv_wgrad_meta<true>);
  m.impl("gdn_fwd", gdn_fwd_meta);
  m.impl("gdn_bwd", gdn_bwd_meta);
  m.impl("gdn_bwd_sum", gdn_bwd_sum_meta);
  m.impl("gdn_fwd_xb", gdn_fwd_xb_meta);
  m.impl("gdn_bwd_sum_xb", gdn_bwd_sum_xb_meta);
  m.impl("gdn_fwd_rn", gdn_fwd_rn_meta);
  m.impl("gdn_bwd_sum_rn", gdn_bwd_sum_rn_meta);
  m.impl("conv2d_fwd_xb", conv2d_fwd_xb_meta);
  m.impl("conv_transpose2d_dgrad_xb", conv_dgrad_xb_meta);
  m.impl("conv2d_dgrad_xb", conv_dgrad_xb_meta);
  m.impl("conv2d_wgrad_xb", conv_wgrad_xb_meta<false>);
  m.impl("conv_transpose2d_wgrad_xb", conv_wgrad_xb_meta<true>);
  m.impl("conv_transpose2d_fwd_xb", conv_transpose2d_fwd_xb_meta);
  m.impl("nonneg_fwd", nonneg_fwd_meta);
  m.impl("nonneg_bwd", nonneg_bwd_meta);
  m.impl("nonneg_multi_fwd", nonneg_multi_fwd_meta);
  m.impl("nonneg_multi_bwd", nonneg_multi_bwd_meta);
  m.impl("bound_fwd", bound_fwd_meta);
  m.impl("bound_bwd", bound_bwd_meta);
  m.impl("relu_fwd", unary_meta);
  m.impl("relu_bwd", binary_meta);
  m.impl("abs_fwd", unary_meta);
  m.impl("abs_bwd", binary_meta);
  m.impl("exp_clamp_fwd", exp_clamp_fwd_meta);
  m.impl("exp_clamp_bwd", exp_clamp_bwd_meta);
  m.impl("ce_loss_fwd", scalar_loss_meta1);
  m.impl("ce_loss_bwd", ce_loss_bwd_meta);
  m.impl("mse_fwd", scalar_loss_meta2);
  m.impl("mse_bwd", pair_grad_meta);
  m.impl("sqdiff_fwd", binary_meta);
  m.impl("sqdiff_bwd", pair_grad_meta);
  m.impl("factorized_fwd", factorized_fwd_meta);
  m.impl("factorized_bwd", factorized_bwd_meta);
  m.impl("factorized_net_fwd", factorized_net_fwd_meta);
  m.impl("factorized_net_bwd", factorized_net_bwd_meta);
  m.impl("quantize", quantize_meta);
  m.impl("conditional_fwd", conditional_fwd_meta);
  m.impl("conditional_bwd", conditional_bwd_meta);
  m.impl("philox_advance", philox_advance_meta);
  m.impl("msssim_fwd", msssim_fwd_meta);
  m.impl("msssim_bwd", msssim_bwd_meta);
}

// The entropy coder's ops live in a namespace of their own: imgcomp holds exactly the training step's launchers.
TORCH_LIBRARY(imgcomp_codec, m) {
  m.def("symbolize(Tensor x) -> (Tensor, int)");
  m.def("scale_index(Tensor sigma, float[] mids) -> Tensor");
  m.def("build_tables(Tensor pmf) -> Tensor");
  m.def("encode(Tensor sym, Tensor? rows, int channels, Tensor tables, int steps_per_chunk) -> Tensor");
  m.def("decode(Tensor packed, int n, Tensor? rows, int channels, Tensor tables, int steps_per_chunk) -> Tensor");
}

TORCH_LIBRARY_IMPL(imgcomp_codec, CUDA, m) {
  m.impl("symbolize", codec_symbolize);
  m.impl("scale_index", codec_scale_index);
  m.impl("build_tables", codec_build_tables);
  m.impl("encode", codec_encode);
  m.impl("decode", codec_decode);
}

TORCH_LIBRARY_IMPL(imgcomp_codec, Meta, m) {
  m.impl("symbolize", codec_symbolize_meta);
  m.impl("scale_index", codec_scale_index_meta);
  m.impl("build_tables", codec_build_tables_meta);
  m.impl("encode", codec_encode_meta);
  m.impl("decode", codec_decode_meta);
}

// The per-image streams' ops (compress_each / decompress_each): additive, in a namespace of their own.
TORCH_LIBRARY(imgcomp_stream, m) {
  m.def("symbolize_seg(Tensor x, int nseg) -> (Tensor, int[])");
  m.def("encode_seg(Tensor sym, int nseg, Tensor? rows, int channels, Tensor pool, int nrows, int[] seg_k, "
        "int[] seg_off, int steps_per_chunk) -> Tensor");
  m.def("decode_seg(Tensor packed, int nseg, int seg_len, Tensor? rows, int channels, Tensor pool, int nrows, "
        "int[] seg_k, int[] seg_off, int steps_per_chunk) -> Tensor");
  m.def("pad_edge(Tensor x, int height, int width) -> Tensor");
  m.def("crop_clamp(Tensor x, int height, int width) -> Tensor");
}

TORCH_LIBRARY_IMPL(imgcomp_stream, CUDA, m) {
  m.impl("symbolize_seg", stream_symbolize_seg);
  m.impl("encode_seg", stream_encode_seg);
  m.impl("decode_seg", stream_decode_seg);
  m.impl("pad_edge", stream_pad_edge);
  m.impl("crop_clamp", stream_crop_clamp);
}

TORCH_LIBRARY_IMPL(imgcomp_stream, Meta, m) {
  m.impl("symbolize_seg", stream_symbolize_seg_meta);
  m.impl("encode_seg", stream_encode_seg_meta);
  m.impl("decode_seg", stream_decode_seg_meta);
  m.impl("pad_edge", stream_pad_edge_meta);
  m.impl("crop_clamp", stream_crop_clamp_meta);
}

// The mean-scale hyperprior's ops (MeanScaleCompressor2018): additive, in a namespace of their own.
TORCH_LIBRARY(imgcomp_mean, m) {
  m.def("symbolize(Tensor y, Tensor mu) -> (Tensor, int)");
  m.def("symbolize_seg(Tensor y, Tensor mu, int nseg) -> (Tensor, int[])");
  m.def("center_round(Tensor y, Tensor mu) -> (Tensor, Tensor)");
  m.def("add_mean(Tensor r, Tensor mu) -> Tensor");
}

TORCH_LIBRARY_IMPL(imgcomp_mean, CUDA, m) {
  m.impl("symbolize", mean_symbolize);
  m.impl("symbolize_seg", mean_symbolize_seg);
  m.impl("center_round", mean_center_round);
  m.impl("add_mean", mean_add);
}

TORCH_LIBRARY_IMPL(imgcomp_mean, Meta, m) {
  m.impl("symbolize", mean_symbolize_meta);
  m.impl("symbolize_seg", mean_symbolize_seg_meta);
  m.impl("center_round", mean_center_round_meta);
  m.impl("add_mean", mean_add_meta);
}

// The checkerboard context model's ops (CheckerboardCompressor2018): additive, in a namespace of their own.
TORCH_LIBRARY(imgcomp_ckbd, m) {
  m.def("input_fwd(Tensor y, Tensor mu) -> (Tensor, Tensor)");
  m.def("input_bwd(Tensor y, Tensor mu, Tensor du, Tensor dv) -> (Tensor, Tensor)");
  m.def("params_fwd(Tensor mu_h, Tensor sigma_h, Tensor a, Tensor b) -> (Tensor, Tensor)");
  m.def("params_bwd(Tensor sigma_h, Tensor b, Tensor dmu, Tensor dsigma) -> (Tensor, Tensor, Tensor, Tensor)");
  m.def("gather(Tensor src, int parity) -> Tensor");
  m.def("scatter(Tensor half, Tensor(a!) full, int parity) -> ()");
}

TORCH_LIBRARY_IMPL(imgcomp_ckbd, CUDA, m) {
  m.impl("input_fwd", ckbd_input_fwd);
  m.impl("input_bwd", ckbd_input_bwd);
  m.impl("params_fwd", ckbd_params_fwd);
  m.impl("params_bwd", ckbd_params_bwd);
  m.impl("gather", ckbd_gather);
  m.impl("scatter", ckbd_scatter);
}

TORCH_LIBRARY_IMPL(imgcomp_ckbd, Meta, m) {
  m.impl("input_fwd", ckbd_input_fwd_meta);
  m.impl("input_bwd", ckbd_input_bwd_meta);
  m.impl("params_fwd", ckbd_params_fwd_meta);
  m.impl("params_bwd", ckbd_params_bwd_meta);
  m.impl("gather", ckbd_gather_meta);
  m.impl("scatter", ckbd_scatter_meta);
}

// The checkerboard context as one batch-invariant kernel (MODEL.CONTEXT.KERNEL "fused"): additive, in a namespace
// of its own.  Inference only: no autograd node.
TORCH_LIBRARY(imgcomp_ctx, m) {
  m.def("context_fwd(Tensor y_in, Tensor mu_h, Tensor sigma_h, Tensor w_mean, Tensor b_mean, Tensor w_scale, "
        "Tensor b_scale) -> (Tensor, Tensor)");
  m.def("context_fwd_ws(Tensor y_in, Tensor mu_h, Tensor sigma_h, Tensor w_mean, Tensor b_mean, Tensor w_scale, "
        "Tensor b_scale, Tensor(a!) ws, bool packed) -> (Tensor, Tensor)");
}

TORCH_LIBRARY_IMPL(imgcomp_ctx, CUDA, m) {
  m.impl("context_fwd", ctx_context_fwd);
  m.impl("context_fwd_ws", ctx_context_fwd_ws);
}

TORCH_LIBRARY_IMPL(imgcomp_ctx, Meta, m) {
  m.impl("context_fwd", ctx_context_fwd_meta);
  m.impl("context_fwd_ws", ctx_context_fwd_ws_meta);
}

// h_s as batch-invariant layers (MODEL.HYPER_SYNTHESIS.KERNEL "invariant"): additive, in a namespace of its own.
// Inference only: no autograd node.
TORCH_LIBRARY(imgcomp_hs, m) {
  m.def("layer(Tensor x, Tensor w, Tensor b, int stride, int epilogue, Tensor? w2, Tensor? b2, int epilogue2, "
        "float lo, float hi) -> (Tensor, Tensor)");
  m.def("layer_ws(Tensor x, Tensor w, Tensor b, int stride, int epilogue, Tensor? w2, Tensor? b2, int epilogue2, "
        "float lo, float hi, Tensor(a!) ws, bool packed) -> (Tensor, Tensor)");
}

TORCH_LIBRARY_IMPL(imgcomp_hs, CUDA, m) {
  m.impl("layer", hs_layer);
  m.impl("layer_ws", hs_layer_ws);
}

TORCH_LIBRARY_IMPL(imgcomp_hs, Meta, m) {
  m.impl("layer", hs_layer_meta);
  m.impl("layer_ws", hs_layer_ws_meta);
}

// The gain units' ops (GainedMeanScaleCompressor2018): additive, in a namespace of their own.
TORCH_LIBRARY(imgcomp_gain, m) {
  m.def("gain_vector(Tensor table, float[] q) -> Tensor");
  m.def("gain_vector_bwd(Tensor g, Tensor dout, int S, float[] q) -> Tensor");
  m.def("channel_scale(Tensor x, Tensor g) -> Tensor");
  m.def("channel_scale_bwd(Tensor x, Tensor g, Tensor dy) -> (Tensor, Tensor)");
}

TORCH_LIBRARY_IMPL(imgcomp_gain, CUDA, m) {
  m.impl("gain_vector", gain_vector);
  m.impl("gain_vector_bwd", gain_vector_bwd);
  m.impl("channel_scale", channel_scale);
  m.impl("channel_scale_bwd", channel_scale_bwd);
}

TORCH_LIBRARY_IMPL(imgcomp_gain, Meta, m) {
  m.impl("gain_vector", gain_vector_meta);
  m.impl("gain_vector_bwd", gain_vector_bwd_meta);
  m.impl("channel_scale", channel_scale_meta);
  m.impl("channel_scale_bwd", channel_scale_bwd_meta);
}

// Region-of-interest coding (RegionGainedMeanScaleCompressor2018): additive, in a namespace of its own.
TORCH_LIBRARY(imgcomp_region, m) {
  m.def("block_scale(Tensor x, Tensor g, Tensor idx, int shift) -> Tensor");
  m.def("block_scale_bwd(Tensor x, Tensor g, Tensor idx, Tensor dy, int shift) -> (Tensor, Tensor)");
  m.def("block_mse_fwd(Tensor a, Tensor b, Tensor w, Tensor idx) -> Tensor");
  m.def("block_mse_bwd(Tensor a, Tensor b, Tensor w, Tensor idx, Tensor gout, bool need_a, bool need_b) -> "
        "(Tensor, Tensor)");
}

TORCH_LIBRARY_IMPL(imgcomp_region, CUDA, m) {
  m.impl("block_scale", block_scale);
  m.impl("block_scale_bwd", block_scale_bwd);
  m.impl("block_mse_fwd", block_mse_fwd);
  m.impl("block_mse_bwd", block_mse_bwd);
}

TORCH_LIBRARY_IMPL(imgcomp_region, Meta, m) {
  m.impl("block_scale", block_scale_meta);
  m.impl("block_scale_bwd", block_scale_bwd_meta);
  m.impl("block_mse_fwd", block_mse_fwd_meta);
  m.impl("block_mse_bwd", block_mse_bwd_meta);
}

// Rate and distortion maps (Compressor2018.rate_distortion_map): additive, in a namespace of their own.
TORCH_LIBRARY(imgcomp_map, m) {
  m.def("block_bits(Tensor p, int shift, Tensor? add=None) -> Tensor");
  m.def("block_sse(Tensor a, Tensor b, int shift) -> Tensor");
}

TORCH_LIBRARY_IMPL(imgcomp_map, CUDA, m) {
  m.impl("block_bits", map_block_bits);
  m.impl("block_sse", map_block_sse);
}

TORCH_LIBRARY_IMPL(imgcomp_map, Meta, m) {
  m.impl("block_bits", map_block_bits_meta);
  m.impl("block_sse", map_block_sse_meta);
}

// Coding to a byte budget (GainedMeanScaleCompressor2018.compress_each_to): additive, in a namespace of its own.
// Inference only: no autograd node.
TORCH_LIBRARY(imgcomp_rate, m) {
  m.def("measure_seg(Tensor sym, int nseg, Tensor? rows, int channels, Tensor pool, int nrows, int[] seg_k, "
        "int[] seg_off, int steps_per_chunk) -> Tensor");
  m.def("gain_symbolize_seg(Tensor y, Tensor g, Tensor mu, int[] img) -> (Tensor, int[])");
}

TORCH_LIBRARY_IMPL(imgcomp_rate, CUDA, m) {
  m.impl("measure_seg", rate_measure_seg);
  m.impl("gain_symbolize_seg", rate_gain_symbolize_seg);
}

TORCH_LIBRARY_IMPL(imgcomp_rate, Meta, m) {
  m.impl("measure_seg", rate_measure_seg_meta);
  m.impl("gain_symbolize_seg", rate_gain_symbolize_seg_meta);
}

// Encode-time latent refinement (Compressor2018.compress_each_refined): additive, in a namespace of its own.
// Inference only: no autograd node.  `update` steps v, m and u in place; `keep` writes best_sym, best and best_step.
TORCH_LIBRARY(imgcomp_refine, m) {
  m.def("update(Tensor(a!) v, Tensor(b!)? m, Tensor(c!)? u, Tensor? g, Tensor? mu, float lr, float c1, float c2) -> "
        "(Tensor, Tensor)");
  m.def("dist_grad(Tensor x, Tensor x_hat, Tensor w) -> Tensor");
  m.def("objective(Tensor bits, Tensor sse, Tensor w) -> Tensor");
  m.def("keep(Tensor sym, Tensor(a!) best_sym, Tensor obj, Tensor(b!) best, Tensor(c!) best_step, int step) -> ()");
  m.def("kmax(Tensor sym, int nseg) -> Tensor");
}

TORCH_LIBRARY_IMPL(imgcomp_refine, CUDA, m) {
  m.impl("update", refine_update);
  m.impl("dist_grad", refine_dist_grad);
  m.impl("objective", refine_objective);
  m.impl("keep", refine_keep);
  m.impl("kmax", refine_kmax);
}

TORCH_LIBRARY_IMPL(imgcomp_refine, Meta, m) {
  m.impl("update", refine_update_meta);
  m.impl("dist_grad", refine_dist_grad_meta);
  m.impl("objective", refine_objective_meta);
  m.impl("keep", refine_keep_meta);
  m.impl("kmax", refine_kmax_meta);
}

// Decoding a pixel window of a per-image stream (Compressor2018.decompress_window): additive, in a namespace of its
// own.  Inference only: no autograd node.
TORCH_LIBRARY(imgcomp_window, m) {
  m.def("decode(Tensor packed, int[] windows, int rh, int rw, int[] spans, Tensor? rows, Tensor? mu, int channels, "
        "Tensor pool, int nrows, int steps_per_chunk) -> Tensor");
  m.def("crop_clamp_at(Tensor x, int top, int left, int height, int width) -> Tensor");
}

TORCH_LIBRARY_IMPL(imgcomp_window, CUDA, m) {
  m.impl("decode", window_decode);
  m.impl("crop_clamp_at", window_crop_clamp_at);
}

TORCH_LIBRARY_IMPL(imgcomp_window, Meta, m) {
  m.impl("decode", window_decode_meta);
  m.impl("crop_clamp_at", window_crop_clamp_at_meta);
}

// Transcoding in the latent domain (Compressor2018.transcode_each, GainedMeanScaleCompressor2018.transcode_each_to):
// additive, in a namespace of its own.  Inference only: no autograd node.
TORCH_LIBRARY(imgcomp_transcode, m) {
  m.def("requant_seg(Tensor r, Tensor mu1, Tensor a, Tensor b, Tensor mu2, int[] img) -> (Tensor, int[])");
}

TORCH_LIBRARY_IMPL(imgcomp_transcode, CUDA, m) { m.impl("requant_seg", transcode_requant_seg); }

TORCH_LIBRARY_IMPL(imgcomp_transcode, Meta, m) { m.impl("requant_seg", transcode_requant_seg_meta); }

// Layered per-image streams (Compressor2018.compress_each_layered / decompress_each_layered): additive, in a namespace
// of its own.  Inference only: no autograd node.
TORCH_LIBRARY(imgcomp_layer, m) {
  m.def("energy(Tensor sym) -> Tensor");
  m.def("gather(Tensor src, int layers, int[] order, int[] seg) -> Tensor");
  m.def("scatter(Tensor q, Tensor? mu, int N, int P, int C, int layers, int[] order, int[] nlayers) -> Tensor");
}

TORCH_LIBRARY_IMPL(imgcomp_layer, CUDA, m) {
  m.impl("energy", layer_energy);
  m.impl("gather", layer_gather);
  m.impl("scatter", layer_scatter);
}

TORCH_LIBRARY_IMPL(imgcomp_layer, Meta, m) {
  m.impl("energy", layer_energy_meta);
  m.impl("gather", layer_gather_meta);
  m.impl("scatter", layer_scatter_meta);
}

// Choosing a quality map under a byte budget (RegionGainedMeanScaleCompressor2018.compress_each_map_to): additive, in a
// namespace of its own.  Inference only: no autograd node.
TORCH_LIBRARY(imgcomp_alloc, m) {
  m.def("block_allocate(Tensor bits, Tensor sse, int[] img, float[] w, int[] codes) -> (Tensor, Tensor, Tensor)");
  m.def("block_gain_symbolize_seg(Tensor y, Tensor g, Tensor rank, Tensor mu, int[] img, int shift) -> (Tensor, int[])");
}

TORCH_LIBRARY_IMPL(imgcomp_alloc, CUDA, m) {
  m.impl("block_allocate", alloc_block_allocate);
  m.impl("block_gain_symbolize_seg", alloc_block_gain_symbolize_seg);
}

TORCH_LIBRARY_IMPL(imgcomp_alloc, Meta, m) {
  m.impl("block_allocate", alloc_block_allocate_meta);
  m.impl("block_gain_symbolize_seg", alloc_block_gain_symbolize_seg_meta);
}
