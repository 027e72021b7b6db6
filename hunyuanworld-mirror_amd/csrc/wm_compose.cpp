// Weights composed from several tensors of a DPT head: built from host copies after a weight change, never per shape and never in the forward.
#include "wm_model.h"

namespace wm_host {

void free_tconv(TconvPack& t) {
  if (t.w16) (void)hipFree(t.w16);
  if (t.bias_rep) (void)hipFree(t.bias_rep);
  if (t.bmiss) (void)hipFree(t.bmiss);
  t = TconvPack();
}
void free_up1comp(Up1Comp& u) {
  if (u.w16) (void)hipFree(u.w16);
  if (u.bias) (void)hipFree(u.bias);
  u = Up1Comp();
}
void free_tapfold(TapFold& t) {
  for (int i = 0; i < 4; ++i) {
    if (t.w16[i]) (void)hipFree(t.w16[i]);
    if (t.bias[i]) (void)hipFree(t.bias[i]);
  }
  t = TapFold();
}

// ---- token-conv: Conv2d(3x3, pad 1, no bias) o ConvTranspose2d(kernel = stride = k) composed at the token resolution (WmGemmArgs::tc_k)
// For output phase (a, b) of token (i, j) the 3x3 taps land in at most two token rows and two token columns:
//   rn[(k i + a, k j + b)] = sum over neighbours (di, dj) of M[a, b, di, dj] p[i + di][j + dj]  +  (sum over taps inside the image of W_rn[tap]) b_ct
//   M[a, b, di, dj] = sum over taps (dy, dx) with floor((a + dy) / k) = di, floor((b + dx) / k) = dj of W_rn[tap] W_ct[(a + dy) mod k][(b + dx) mod k]
// 36 (phase, neighbour) matrices for k = 4, 16 for k = 2, instead of k^2 x 9 tap products per token: 4.4x / 2.7x fewer flops than ConvTranspose
// GEMM + 3x3 conv, no ConvTranspose output tensor, one rounding of the combined weight instead of two operand roundings.
// wct: torch ConvTranspose2d weight [Cin][Cm][k][k], bct [Cm], wrn: torch Conv2d weight [F][Cm][3][3] (host fp32).  F must be 256.
hipError_t build_tconv(int dt, int k, int Cin, int Cm, int F_, const float* wct, const float* bct, const float* wrn, TconvPack& out, hipStream_t s) {
  if (F_ != 256 || (k != 2 && k != 4) || Cin % 64 || Cm % 4) return hipErrorInvalidValue;
  free_tconv(out);
  out.k = k; out.cin = Cin;
  const int k2 = k * k;
  std::vector<float> a_tap((size_t)9 * F_ * Cm), b_ph((size_t)k2 * Cin * Cm);
  for (int f = 0; f < F_; ++f)
    for (int c = 0; c < Cm; ++c)
      for (int t = 0; t < 9; ++t) a_tap[((size_t)t * F_ + f) * Cm + c] = wrn[((size_t)f * Cm + c) * 9 + t];
  for (int ci = 0; ci < Cin; ++ci)
    for (int c = 0; c < Cm; ++c)
      for (int ph = 0; ph < k2; ++ph) b_ph[((size_t)ph * Cin + ci) * Cm + c] = wct[((size_t)ci * Cm + c) * k2 + ph];
  float *d_a = nullptr, *d_b = nullptr, *d_bct = nullptr, *d_m = nullptr;
  hipError_t e;
#define TC(x) do { e = (x); if (e != hipSuccess) goto done; } while (0)
  TC(hipMalloc((void**)&d_a, a_tap.size() * 4));
  TC(hipMalloc((void**)&d_b, b_ph.size() * 4));
  TC(hipMalloc((void**)&d_bct, (size_t)Cm * 4));
  TC(hipMalloc((void**)&d_m, (size_t)F_ * Cin * 4));
  TC(hipMalloc(&out.w16, (size_t)k2 * 256 * 4 * Cin * 2));
  TC(hipMalloc((void**)&out.bias_rep, (size_t)k2 * 256 * 4));
  TC(hipMalloc((void**)&out.bmiss, (size_t)9 * 256 * 4));
  TC(hipMemcpyAsync(d_a, a_tap.data(), a_tap.size() * 4, hipMemcpyHostToDevice, s));
  TC(hipMemcpyAsync(d_b, b_ph.data(), b_ph.size() * 4, hipMemcpyHostToDevice, s));
  TC(hipMemcpyAsync(d_bct, bct, (size_t)Cm * 4, hipMemcpyHostToDevice, s));
  TC(hipMemsetAsync(out.w16, 0, (size_t)k2 * 256 * 4 * Cin * 2, s));
  for (int a = 0; a < k; ++a)
    for (int b = 0; b < k; ++b) {
      const int ph = a * k + b;
      unsigned word = 0;
      int idx = 0;
      for (int di = -1; di <= 1; ++di)
        for (int dj = -1; dj <= 1; ++dj) {
          bool first = true;
          for (int dy = -1; dy <= 1; ++dy)
            for (int dx = -1; dx <= 1; ++dx) {
              const int ya = a + dy, xb = b + dx;
              const int fi = ya < 0 ? -1 : ya / k, fj = xb < 0 ? -1 : xb / k;   // floor
              if (fi != di || fj != dj) continue;
              const int pa = ((ya % k) + k) % k, pb = ((xb % k) + k) % k;
              TC(wm_launch_linear_f32(d_a + (size_t)((dy + 1) * 3 + dx + 1) * F_ * Cm, d_b + (size_t)(pa * k + pb) * Cin * Cm, nullptr, d_m, F_, Cin, Cm, Cm,
                                      Cin, 0, 0, nullptr, first ? 0 : 1, s));
              first = false;
            }
          if (first) continue;   // no tap of this phase lands in that neighbour
          TC(wm_launch_f32_to_16_2d(d_m, Cin, (uint16_t*)out.w16 + (size_t)ph * 256 * 4 * Cin + (size_t)idx * Cin, 4 * Cin, F_, Cin, dt, s));
          word |= (unsigned)((di + 1) | ((dj + 1) << 2)) << (4 * idx);
          ++idx;
        }
      out.list[ph] = word | ((unsigned)idx << 16);
    }
  for (int t = 0; t < 9; ++t)   // bmiss[t] = W_rn[t] b_ct ; bias = their sum
    TC(wm_launch_linear_f32(d_bct, d_a + (size_t)t * F_ * Cm, nullptr, out.bmiss + (size_t)t * 256, 1, F_, Cm, Cm, F_, 0, 0, nullptr, 0, s));
  for (int t = 0; t < 9; ++t)
    TC(wm_launch_linear_f32(d_bct, d_a + (size_t)t * F_ * Cm, nullptr, out.bias_rep, 1, F_, Cm, Cm, F_, 0, 0, nullptr, t ? 1 : 0, s));
  for (int ph = 1; ph < k2; ++ph) TC(hipMemcpyAsync(out.bias_rep + (size_t)ph * 256, out.bias_rep, 256 * 4, hipMemcpyDeviceToDevice, s));
  TC(hipStreamSynchronize(s));
#undef TC
done:
  if (d_a) (void)hipFree(d_a);
  if (d_b) (void)hipFree(d_b);
  if (d_bct) (void)hipFree(d_bct);
  if (d_m) (void)hipFree(d_m);
  if (e != hipSuccess) free_tconv(out);
  return e;
}
// woc1: torch Conv2d weight [Co][F][3][3]; wout: [F][F] (1x1); bout [F] (host fp32)
static hipError_t build_up1comp(int dt, int F_, int Co, const float* woc1, const float* wout, const float* bout, Up1Comp& out, hipStream_t s) {
  free_up1comp(out);
  out.co = Co;
  std::vector<float> a_tap((size_t)9 * Co * F_), wt((size_t)F_ * F_);
  for (int co = 0; co < Co; ++co)
    for (int c = 0; c < F_; ++c)
      for (int t = 0; t < 9; ++t) a_tap[((size_t)t * Co + co) * F_ + c] = woc1[((size_t)co * F_ + c) * 9 + t];
  for (int c = 0; c < F_; ++c)
    for (int ci = 0; ci < F_; ++ci) wt[(size_t)ci * F_ + c] = wout[(size_t)c * F_ + ci];   // W_out^T: rows ci, K = c
  float *d_a = nullptr, *d_w = nullptr, *d_b = nullptr, *d_m = nullptr;
  hipError_t e;
#define TC(x) do { e = (x); if (e != hipSuccess) goto done; } while (0)
  TC(hipMalloc((void**)&d_a, a_tap.size() * 4));
  TC(hipMalloc((void**)&d_w, wt.size() * 4));
  TC(hipMalloc((void**)&d_b, (size_t)F_ * 4));
  TC(hipMalloc((void**)&d_m, (size_t)9 * Co * F_ * 4));
  TC(hipMalloc(&out.w16, (size_t)9 * Co * F_ * 2));
  TC(hipMalloc((void**)&out.bias, (size_t)9 * Co * 4));
  TC(hipMemcpyAsync(d_a, a_tap.data(), a_tap.size() * 4, hipMemcpyHostToDevice, s));
  TC(hipMemcpyAsync(d_w, wt.data(), wt.size() * 4, hipMemcpyHostToDevice, s));
  TC(hipMemcpyAsync(d_b, bout, (size_t)F_ * 4, hipMemcpyHostToDevice, s));
  // all nine taps at once: rows (tap, co) of a_tap against W_out^T -> [9 Co][F]; the bias rows the same against b_out
  TC(wm_launch_linear_f32(d_a, d_w, nullptr, d_m, 9 * Co, F_, F_, F_, F_, 0, 0, nullptr, 0, s));
  TC(wm_launch_f32_to_16_2d(d_m, F_, out.w16, F_, 9 * Co, F_, dt, s));
  TC(wm_launch_linear_f32(d_b, d_a, nullptr, out.bias, 1, 9 * Co, F_, F_, 9 * Co, 0, 0, nullptr, 0, s));
  TC(hipStreamSynchronize(s));
#undef TC
done:
  if (d_a) (void)hipFree(d_a);
  if (d_w) (void)hipFree(d_w);
  if (d_b) (void)hipFree(d_b);
  if (d_m) (void)hipFree(d_m);
  if (e != hipSuccess) free_up1comp(out);
  return e;
}
hipError_t build_tapfold(int dt, int nh, int oc, int K, int Kp, const float* const* Wh, const float* const* bh, const float* const* gamma,
                                const float* const* beta, void** w16_out, float** bias_out, bool* in_range) {
  // fp64 on the host, one rounding to the operand type
  *w16_out = nullptr; *bias_out = nullptr; *in_range = true;
  std::vector<uint16_t> w16((size_t)nh * oc * Kp, 0);
  std::vector<float> bias((size_t)nh * oc);
  for (int hd = 0; hd < nh; ++hd)
    for (int r = 0; r < oc; ++r) {
      const float* wr = Wh[hd] + (size_t)r * K;
      double acc = (double)bh[hd][r];
      uint16_t* o = &w16[((size_t)hd * oc + r) * Kp];
      for (int k = 0; k < K; ++k) {
        const float wf = (float)((double)wr[k] * (double)gamma[hd][k]);
        if (!std::isfinite(wf) || (dt == WM_DT_F16 && std::fabs(wf) > 65504.0f) || (dt == WM_DT_BF16 && std::fabs(wf) > 3.3895314e38f)) *in_range = false;
        o[k] = h_to16(wf, dt);
        acc += (double)wr[k] * (double)beta[hd][k];
      }
      bias[(size_t)hd * oc + r] = (float)acc;
      if (!std::isfinite(bias[(size_t)hd * oc + r])) *in_range = false;
    }
  if (!*in_range) return hipSuccess;
  hipError_t e = hipMalloc(w16_out, w16.size() * 2);
  if (e == hipSuccess) e = hipMalloc((void**)bias_out, bias.size() * 4);
  if (e == hipSuccess) e = hipMemcpy(*w16_out, w16.data(), w16.size() * 2, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(*bias_out, bias.data(), bias.size() * 4, hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    if (*w16_out) (void)hipFree(*w16_out);
    if (*bias_out) (void)hipFree(*bias_out);
    *w16_out = nullptr; *bias_out = nullptr;
  }
  return e;
}

// rn = tconv(tokens): tokens16 [n][gh][gw][Cin] (16-bit) -> out fp32 [n][k gh][k gw][256]
hipError_t launch_tconv(const TconvPack& t, int dt, const void* tokens16, float* out, int n, int gh, int gw, const void* zero16, hipStream_t s) {
  WmGemmArgs g;
  memset(&g, 0, sizeof(g));
  g.A = tokens16; g.W = t.w16; g.C = out; g.bias = t.bias_rep; g.M = n * gh * gw; g.N = t.k * t.k * 256; g.K = 4 * t.cin; g.lda = t.cin; g.ldw = 4 * t.cin; g.ldc = 256;
  g.dtype = dt; g.epi = WM_EPI_CONV; g.cv_h = gh; g.cv_w = gw; g.cv_cin = t.cin; g.cv_zero = zero16; g.tc_k = t.k;
  memcpy(g.tc_list, t.list, sizeof(g.tc_list));
  hipError_t e = wm_launch_gemm(g, s);
  if (e != hipSuccess) return e;
  return wm_launch_tconv_border(out, t.bmiss, n, t.k * gh, t.k * gw, 256, s);
}

// Everything above, rebuilt for the handle's heads when a weight has changed since the last plan (plan() calls this for every new shape)
wm_status rebuild_weight_derived(wm_handle* h, const Dims& d) {
  const wm_config& c = h->cfg;
  // the composed ConvTranspose -> layer_rn GEMMs of the DPT heads (weight-derived only: rebuilt after a weight change, not per shape)
  if (!h->tconv_valid) {
    for (auto& hd : h->tconv) for (TconvPack& t : hd) free_tconv(t);
    for (Up1Comp& u : h->up1comp) free_up1comp(u);
    if (c.dpt_features == 256)
      for (int id = HD_DEPTH; id <= HD_NORM; ++id)
        for (int i = 0; i < 2 && head_enabled(c, id); ++i) {
          const std::string p = kHeadPrefix[id];
          const Weight* wct = W(h, p + "resize_layers." + std::to_string(i) + ".weight");
          const Weight* bct = W(h, p + "resize_layers." + std::to_string(i) + ".bias");
          const Weight* wrn = W(h, p + "scratch.layer" + std::to_string(i + 1) + "_rn.weight");
          const int k = i == 0 ? 4 : 2, oc = c.dpt_out_channels[i];
          if (!wct || !bct || !wrn || wct->host.empty() || bct->host.empty() || wrn->host.empty() || oc % 64) continue;
          if (wct->host.size() != (size_t)oc * oc * k * k || bct->host.size() != (size_t)oc || wrn->host.size() != (size_t)256 * oc * 9) continue;
          HIPCHK(h, build_tconv(c.head_dtype, k, oc, oc, 256, wct->host.data(), bct->host.data(), wrn->host.data(), h->tconv[id][i], nullptr));
        }
    if (c.head_dtype == WM_DT_F16)
      for (int id = HD_DEPTH; id <= HD_NORM; ++id) {
        if (!head_enabled(c, id)) continue;
        const std::string p = kHeadPrefix[id];
        const Weight* w1 = W(h, p + "scratch.output_conv1.weight");
        const Weight* wo = W(h, p + "scratch.refinenet1.out_conv.weight");
        const Weight* bo = W(h, p + "scratch.refinenet1.out_conv.bias");
        const int F_ = c.dpt_features;
        if (!w1 || !wo || !bo || w1->host.empty() || wo->host.empty() || bo->host.empty() || F_ % 64 || w1->shape.size() != 4) continue;
        const int Co = (int)w1->shape[0];
        if ((Co != 128 && Co != 64 && Co != 32) || w1->host.size() != (size_t)Co * F_ * 9 || wo->host.size() != (size_t)F_ * F_ || bo->host.size() != (size_t)F_) continue;
        HIPCHK(h, build_up1comp(c.head_dtype, F_, Co, w1->host.data(), wo->host.data(), bo->host.data(), h->up1comp[id], nullptr));
      }
    // the heads' shared tap front: every enabled DPT head reads the same four taps through a LayerNorm(2D) and 1x1 projections of the same widths
    free_tapfold(h->tapfold);
    {
      TapFold tf;   // heads in the order the forward runs them (and numbers their workspace slots)
      for (int id = 0; id < HD_COUNT; ++id)
        if (head_enabled(c, id)) tf.heads[tf.nh++] = id;
      const int D2 = 2 * d.D, Kp = ru(D2, 64);
      bool ok = tf.nh >= 2;
      std::vector<const float*> Wh, bh, gm, bt;
      for (int i = 0; i < 4 && ok; ++i) {
        const int oci = c.dpt_out_channels[i];
        Wh.clear(); bh.clear(); gm.clear(); bt.clear();
        for (int k = 0; k < tf.nh; ++k) {
          const std::string p = kHeadPrefix[tf.heads[k]];
          const Weight* w = W(h, p + "projects." + std::to_string(i) + ".weight");
          const Weight* b = W(h, p + "projects." + std::to_string(i) + ".bias");
          const Weight* g = W(h, p + "norm.weight");
          const Weight* e = W(h, p + "norm.bias");
          // (a head whose tensors are missing or of another size keeps the whole group on the direct form)
          if (!w || !b || !g || !e || w->host.size() != (size_t)oci * D2 || b->host.size() != (size_t)oci || g->host.size() != (size_t)D2 ||
              e->host.size() != (size_t)D2 || w->k16 != Kp || (oci & 3)) { ok = false; break; }
          Wh.push_back(w->host.data()); bh.push_back(b->host.data()); gm.push_back(g->host.data()); bt.push_back(e->host.data());
        }
        if (!ok) break;
        bool in_range = false;
        HIPCHK(h, build_tapfold(c.head_dtype, tf.nh, oci, D2, Kp, Wh.data(), bh.data(), gm.data(), bt.data(), &tf.w16[i], &tf.bias[i], &in_range));
        if (!in_range) ok = false;   // gamma now scales a weight: out of the operand type's range -> the direct form for this handle
      }
      if (ok) { tf.valid = true; h->tapfold = tf; }
      else free_tapfold(tf);
    }
    h->tconv_valid = true;
  }
  return WM_OK;
}

}  // namespace wm_host
