// The camera head and the DPT heads of the forward.
#include "wm_model.h"

namespace wm_host {

wm_status linear32(Ctx& c, const float* X, int ldx, const Lin32& w, float* Y, int ldy, int M, int pre, int post,
                   const float* gamma, int accumulate) {
  LCHK(c, wm_launch_linear_f32(X, w.w, w.b, Y, M, w.N, w.K, ldx, ldy, pre, post, gamma, accumulate, c.s));
  return WM_OK;
}

// CameraHead.forward (camera_head.py:58-104) on all nt views, fp32
wm_status camera_head(Ctx& c, float* out_params) {
  wm_handle* h = c.h;
  const Dims& d = c.d;
  const wm_config& cf = h->cfg;
  const Model& m = h->m;
  const Workspace& ws = h->ws;
  const int D2 = 2 * d.D, S = d.nt;
  float* tok = ws.cam_tok;
  wm_status st;
  // token_norm on tap3[:, :, 0]
  float* tok_local = d.world > 1 ? ws.cam_tok_local : tok;
  WmLnArgs ln{};
  ln.x = ws.tap[3]; ln.ld_in = D2; ln.y = tok_local; ln.ld_out = D2; ln.w = m.cam_token_norm.w; ln.b = m.cam_token_norm.b; ln.D = D2; ln.eps = 1e-5f;
  ln.groups = d.n; ln.rows_per_group = 1; ln.in_group = d.P; ln.out_group = 1; ln.out_f32 = 1;
  st = layernorm(c, ln);
  if (st) return st;
  if (d.world > 1) {
    st = comm_allgather(h, tok_local, tok, (size_t)d.n * D2 * 4, c.s);
    if (st) return st;
  }
  float *e = ws.cam_e, *mod = ws.cam_mod, *hh = ws.cam_h, *a = ws.cam_a;
  float *qkv = ws.cam_qkv, *o = ws.cam_o, *f = ws.cam_f;
  float *pred = ws.cam_pred, *delta = ws.cam_delta, *init = ws.cam_init;
  LCHK(c, hipMemsetAsync(pred, 0, (size_t)S * 12 * 4, c.s));
  LCHK(c, hipMemsetAsync(delta, 0, (size_t)S * 12 * 4, c.s));
  ln = WmLnArgs{};   // the trunk's norms: the S rows of hh into a, fp32
  ln.x = hh; ln.ld_in = D2; ln.y = a; ln.ld_out = D2; ln.D = D2; ln.eps = 1e-5f; ln.groups = 1; ln.rows_per_group = S; ln.out_f32 = 1;
  for (int step = 0; step < cf.cam_steps; ++step) {
    st = linear32(c, step == 0 ? init : pred, 12, m.cam_param_embed, e, D2, S, 0, 0);
    if (st) return st;
    st = linear32(c, e, D2, m.cam_adapt, mod, 3 * D2, S, 1, 0);
    if (st) return st;
    LCHK(c, wm_launch_adaln(tok, mod, hh, S, D2, 1e-6f, c.s));
    for (const CamBlockW& w : m.cam) {
      ln.w = w.norm1.w; ln.b = w.norm1.b;
      st = layernorm(c, ln);
      if (st) return st;
      st = linear32(c, a, D2, w.qkv, qkv, 3 * D2, S, 0, 0);
      if (st) return st;
      LCHK(c, wm_launch_small_attention(qkv, o, S, cf.cam_heads, D2 / cf.cam_heads, c.s));
      st = linear32(c, o, D2, w.proj, hh, D2, S, 0, 0, w.ls1, 1);
      if (st) return st;
      ln.w = w.norm2.w; ln.b = w.norm2.b;
      st = layernorm(c, ln);
      if (st) return st;
      st = linear32(c, a, D2, w.fc1, f, 4 * D2, S, 0, 2);
      if (st) return st;
      st = linear32(c, f, 4 * D2, w.fc2, hh, D2, S, 0, 0, w.ls2, 1);
      if (st) return st;
    }
    ln.w = m.cam_out_norm.w; ln.b = m.cam_out_norm.b;
    st = layernorm(c, ln);
    if (st) return st;
    st = linear32(c, a, D2, m.cam_pred_fc1, f, D2 / 2, S, 0, 2);
    if (st) return st;
    st = linear32(c, f, D2 / 2, m.cam_pred_fc2, delta, 12, S, 0, 0);
    if (st) return st;
    LCHK(c, wm_launch_cam_update(pred, delta, out_params, S, step == 0, c.s));
  }
  return WM_OK;
}

// One tap of the shared front for n views: xhat = LayerNorm without affine of the tap's patch rows (hw of P per view, from row psi) as a 16-bit
// tensor, then ONE projection GEMM over all heads' folded rows; head k's oc columns (+ the tap's position table, dense_head.py:204-208) land in
// dst[k] [n hw][oc], 16-bit (out16) or fp32
wm_status tap_front_one(Ctx& c, const float* tap, void* xhat, const void* w16, const float* bias, const float* pos, int nh, int oc, int out16,
                        void* const* dst, int n, int hw, int P, int psi, int D2) {
  WmLnArgs ln{};   // no affine: it is folded into the projection
  ln.x = tap; ln.ld_in = D2; ln.y = xhat; ln.ld_out = D2; ln.D = D2; ln.eps = 1e-5f;
  ln.groups = n; ln.rows_per_group = hw; ln.in_group = P; ln.in_off = psi; ln.out_group = hw; ln.dtype = c.hdt;
  wm_status st = layernorm(c, ln);
  if (st) return st;
  WmGemmArgs ex;
  memset(&ex, 0, sizeof(ex));
  ex.rows_per_group = hw; ex.out_group = hw; ex.out_off = 0; ex.add = pos; ex.out16 = out16;
  ex.split_n = oc;
  for (int k = 0; k < nh; ++k) ex.split_C[k] = dst[k];
  return gemm(c, c.hdt, WM_EPI_ROWMAP_ADD, xhat, D2, w16, ru(D2, 64), nullptr, oc, bias, nullptr, n * hw, nh * oc, D2, &ex);
}

// where head slot `hb` finds the projection of tap i for the views from v0 on (the shared front's outputs; all n views of the rank)
static void* tap_front_dst(const wm_handle* h, const Dims& d, const HeadBufs& hb, int i, int v0) {
  const int32_t* oc = h->cfg.dpt_out_channels;
  void* const base[4] = {hb.P16, hb.P16b, hb.f2, hb.f3in};
  return (char*)base[i] + (size_t)v0 * d.hw * oc[i] * (i < 2 ? 2 : 4);
}

// the shared front of all heads of the group, every view chunk, on c.s (before the heads fork)
wm_status tap_front(Ctx& c) {
  wm_handle* h = c.h;
  const Dims& d = c.d;
  const Workspace& ws = h->ws;
  const TapFold& tf = h->tapfold;
  const int D2 = 2 * d.D, nh = tf.nh;
  void* xhat = ws.hb[0].T16;
  for (int v0 = 0; v0 < d.n; v0 += d.chunk) {
    const int n = std::min(d.chunk, d.n - v0);
    for (int i = 0; i < 4; ++i) {
      void* dst[4] = {nullptr, nullptr, nullptr, nullptr};
      for (int k = 0; k < nh; ++k) dst[k] = tap_front_dst(h, d, ws.hb[k], i, v0);
      const float* tap = ws.tap[i] + (size_t)v0 * d.P * D2;
      wm_status st = tap_front_one(c, tap, xhat, tf.w16[i], tf.bias[i], ws.dpt_pos[i], nh,
                                   h->cfg.dpt_out_channels[i], i < 2 ? 1 : 0, dst, n, d.hw, d.P, d.psi, D2);
      if (st) return st;
    }
  }
  return WM_OK;
}

// the geometry of a conv launch; the caller then sets, by field name, whatever else differs from zero (residuals, ReLUs, 16-bit forms, fused resize)
static WmConvArgs conv_args(const float* x, float* y, int N, int Hi, int Wi, int ksize, int stride, int pad) {
  WmConvArgs a;
  memset(&a, 0, sizeof(a));
  a.x = x; a.y = y; a.N = N; a.Hi = Hi; a.Wi = Wi; a.ksize = ksize; a.stride = stride; a.pad = pad;
  return a;
}

// a.up_hs > 0: x is [N][up_hs][up_ws][Cin] and the conv runs on its align_corners bilinear resize to (Hi, Wi)
// (+ position tables), fused into the 3x3 halo kernel's input staging.
// The weight, bias, channel counts, output size and operand type are filled in here.
static wm_status conv(Ctx& c, const ConvW& w, WmConvArgs a, bool* out16 = nullptr) {
  a.w = w.w16; a.bias = w.bias; a.Cin = w.cin; a.Cout = w.cout; a.dtype = c.hdt;
  a.Ho = (a.Hi + 2 * a.pad - a.ksize) / a.stride + 1; a.Wo = (a.Wi + 2 * a.pad - a.ksize) / a.stride + 1;
  if (out16) {  // the caller can take y as a 16-bit tensor (its only consumer rounds it to the operand type anyway): granted when the kernel can
    *out16 = wm_conv3x3_out16_ok(a);
    a.out16 = *out16 ? 1 : 0;
  }
  // timing kinds by kernel instantiation: the F -> F 3x3 convs of the two large pyramid levels, output_conv1 with its fused
  // resize; everything else (small levels, 1x1, stride 2) under PK_CONV
  const bool pyr = a.ksize == 3 && a.stride == 1 && a.up_hs == 0 && a.Cin == a.Cout && a.Cin >= 128;
  const int kind = a.up_hs > 0 ? PK_OC1_UP : pyr && a.Hi == 4 * c.d.gh ? PK_CONV_4X : pyr && a.Hi == 2 * c.d.gh ? PK_CONV_2X : PK_CONV;
  ProfScope ps(c.h, kind, c.s);
  if (wm_tune(WM_TUNE_CONV_GEMM, 0) == 1 && a.in16 && a.ksize == 3 && a.stride == 1 && a.pad == 1 && a.up_hs == 0 && a.Cin % 64 == 0 && a.Cout % 8 == 0 &&
      (long)a.N * a.Hi * a.Wi >= 4096) {
    // a 16-bit NHWC input: the conv IS the ping-pong GEMM over (pixels) x (tap, channel), the A pieces DMA-ed from the shifted pixels
    WmGemmArgs g;
    memset(&g, 0, sizeof(g));
    g.A = a.x; g.W = a.w; g.C = a.y; g.bias = a.bias; g.M = a.N * a.Hi * a.Wi; g.N = a.Cout; g.K = 9 * a.Cin; g.lda = a.Cin; g.ldw = 9 * a.Cin; g.ldc = a.Cout;
    g.dtype = c.hdt; g.epi = WM_EPI_CONV; g.cv_h = a.Hi; g.cv_w = a.Wi; g.cv_cin = a.Cin; g.cv_zero = c.h->ws.ZERO256;
    g.cv_resid = a.resid; g.cv_resid2 = a.resid2; g.cv_resid_relu = a.resid_relu ? 1 : 0; g.out16 = a.out16; g.relu = a.relu_out;
    LCHK(c, wm_launch_gemm(g, c.s));
    return WM_OK;
  }
  LCHK(c, wm_launch_conv(a, c.s));
  return WM_OK;
}

// ResidualConvUnit (dense_head.py:435-455): y = conv2(relu(conv1(relu x))) + relu(x) (+ extra); w: the unit's conv1, conv2
// y16: when non-null the caller can take y as a 16-bit tensor; *y16 tells whether it got one
// conv1's output has ONE consumer, conv2's input staging, which applies ReLU and rounds to the operand type: where the kernel can, conv1
// writes exactly that — relu(conv1) as a 16-bit tensor — and conv2 stages it unconverted (bit-identical values; a quarter of the
// bytes written, a quarter read: 268 MB less traffic per RCU at 148^2 x 8 views).  Tuning rcu_mid16 = 0: the fp32 intermediate (A/B).
static wm_status rcu(Ctx& c, const ConvW (&w)[2], const float* x, const float* extra, float* tmp, float* y, int N, int Hh, int Ww, bool* y16 = nullptr) {
  const bool want = wm_tune(WM_TUNE_RCU_MID16, 1) != 0;
  bool mid16 = false;
  WmConvArgs a1 = conv_args(x, tmp, N, Hh, Ww, 3, 1, 1);
  a1.relu_in = 1; a1.relu_out = want ? 1 : 0;
  wm_status st = conv(c, w[0], a1, want ? &mid16 : nullptr);
  if (st) return st;
  // (relu_out was requested together with out16; if the kernel could not grant out16 the fp32 tmp holds relu(conv1), and relu is idempotent)
  WmConvArgs a2 = conv_args(tmp, y, N, Hh, Ww, 3, 1, 1);
  a2.resid = x; a2.resid_relu = 1; a2.resid2 = extra; a2.relu_in = mid16 ? 0 : 1; a2.in16 = mid16 ? 1 : 0;
  return conv(c, w[1], a2, y16);
}

// FeatureFusionBlock.out_conv (1x1, dense_head.py:496) on x2 [N*H*W][F]: a plain GEMM when x2 came as a 16-bit tensor (the ping-pong
// kernel, fp32 NHWC out), the generic conv kernel on the fp32 tensor otherwise
// y16: the output as a 16-bit tensor of the operand type (its only consumer is a GEMM: the tap GEMM of upconv.hip); needs x2_is_16
static wm_status out_conv(Ctx& c, const ConvW& w, const float* x2, bool x2_is_16, float* y, int N, int Hh, int Ww, int F_, bool y16 = false) {
  if (!x2_is_16) return y16 ? fail(c.h, WM_ERR_STATE, "out_conv: 16-bit output needs the 16-bit input") : conv(c, w, conv_args(x2, y, N, Hh, Ww, 1, 1, 0));
  return gemm(c, c.hdt, y16 ? WM_EPI_T16 : WM_EPI_F32, x2, F_, w.w16, F_, y, F_, w.bias, nullptr, N * Hh * Ww, F_, F_, nullptr, PK_CONV);
}

// the three of a head slot's four scratch tensors S0..S3 that are not `cur`, in their order
static void others_than(float* const (&S)[4], const float* cur, float* (&others)[3]) {
  int k = 0;
  for (float* b : S) if (b != cur) others[k++] = b;
}

// DPTHead (dense_head.py:107-295) for views [v0, v0+n) of this rank: head `id` (its weights) in workspace slot `slot` (its buffers)
wm_status dpt_head(Ctx& c, int id, int F_, int out_dim, int act, float* out_attr, float* out_conf,
                   const float* img, const wm_outputs* out, int first_view, int slot, bool front_done) {
  // front_done: the shared front (tap_front) has already normalised and projected the four taps of every view for this head's slot
  wm_handle* h = c.h;
  const Dims& d = c.d;
  const wm_config& cf = h->cfg;
  const HeadW& w = h->m.head[id];
  const Workspace& ws = h->ws;
  const HeadBufs& hb = ws.hb[slot];
  const bool is_gs = id == HD_GS;
  const int D2 = 2 * d.D, hw = d.hw, gh = d.gh, gw = d.gw;
  const int32_t* oc = cf.dpt_out_channels;
  float* S0 = hb.s[0]; float* S1 = hb.s[1]; float* S2 = hb.s[2];
  wm_status st;
  for (int v0 = 0; v0 < d.n; v0 += d.chunk) {
    const int n = std::min(d.chunk, d.n - v0);
    float* feats[4] = {hb.f0, hb.f1, front_done ? (float*)tap_front_dst(h, d, hb, 2, v0) : hb.f2, hb.f3};
    bool tconv_done[4] = {false, false, false, false};
    for (int i = 0; i < 4; ++i) {
      const float* tap = ws.tap[i] + (size_t)v0 * d.P * D2;
      void* T16 = hb.T16;
      if (!front_done) {
        WmLnArgs ln{};
        ln.x = tap; ln.ld_in = D2; ln.y = T16; ln.ld_out = D2; ln.w = w.norm.w; ln.b = w.norm.b; ln.D = D2; ln.eps = 1e-5f;
        ln.groups = n; ln.rows_per_group = hw; ln.in_group = d.P; ln.in_off = d.psi; ln.out_group = hw; ln.dtype = c.hdt;
        st = layernorm(c, ln);
        if (st) return st;
      }
      WmGemmArgs ex;
      memset(&ex, 0, sizeof(ex));
      ex.rows_per_group = hw; ex.out_group = hw; ex.out_off = 0; ex.add = ws.dpt_pos[i];
      if (i < 2) {  // feeds a k==stride ConvTranspose (GEMM): 16-bit output
        ex.out16 = 1;
        void* P16 = front_done ? tap_front_dst(h, d, hb, i, v0) : hb.P16;
        if (!front_done) {
          st = gemm(c, c.hdt, WM_EPI_ROWMAP_ADD, T16, D2, w.proj[i].w, D2, P16, oc[i], w.proj[i].b, nullptr, n * hw, oc[i], D2, &ex);
          if (st) return st;
        }
        tconv_done[i] = wm_tune(WM_TUNE_TCONV, 1) != 0 && !is_gs && F_ == 256 && w.tconv[i] != nullptr;
        if (tconv_done[i]) {   // ConvTranspose and layer{i+1}_rn as one GEMM at the token resolution, straight into rn[i]
          ProfScope ps(h, i == 0 ? PK_CONV_4X : PK_CONV, c.s);
          LCHK(c, launch_tconv(*w.tconv[i], c.hdt, P16, hb.rn[i], n, gh, gw, ws.ZERO256, c.s));
          continue;
        }
        const int k = i == 0 ? 4 : 2;
        WmGemmArgs ct;
        memset(&ct, 0, sizeof(ct));
        ct.ct_k = k; ct.ct_cout = oc[i]; ct.ct_gh = gh; ct.ct_gw = gw;
        st = gemm(c, c.hdt, WM_EPI_CONVT, P16, oc[i], w.resize[i].w, oc[i], feats[i], 0, w.resize[i].b, nullptr, n * hw, k * k * oc[i], oc[i], &ct);
        if (st) return st;
      } else {
        float* dst = i == 2 ? feats[2] : front_done ? (float*)tap_front_dst(h, d, hb, 3, v0) : hb.f3in;
        if (!front_done) {
          st = gemm(c, c.hdt, WM_EPI_ROWMAP_ADD, T16, D2, w.proj[i].w, D2, dst, oc[i], w.proj[i].b, nullptr, n * hw, oc[i], D2, &ex);
          if (st) return st;
        }
        if (i == 3) {
          st = conv(c, w.resize3, conv_args(dst, feats[3], n, gh, gw, 3, 2, 1));
          if (st) return st;
        }
      }
    }
    const int Hs[4] = {4 * gh, 2 * gh, gh, d.gh2}, Ws[4] = {4 * gw, 2 * gw, gw, d.gw2};
    float* const* rn = hb.rn;
    for (int i = 0; i < 4; ++i) {
      if (tconv_done[i]) continue;
      st = conv(c, w.rn[i], conv_args(feats[i], rn[i], n, Hs[i], Ws[i], 3, 1, 1));
      if (st) return st;
    }
    // refinenet4: RCU2(rn4) -> resize to level 3 -> out_conv
    bool x16 = false;
    st = rcu(c, w.rcu[3][1], rn[3], nullptr, S0, S1, n, Hs[3], Ws[3], &x16);
    if (st) return st;
    // out_conv (1x1) and the align_corners bilinear resize are both linear and the interpolation weights sum
    // to 1, so out_conv(resize(x)) == resize(out_conv(x)): run the 1x1 at the LOW resolution (4x fewer FLOPs)
    st = out_conv(c, w.out_conv[3], S1, x16, S0, n, Hs[3], Ws[3], F_);
    if (st) return st;
    LCHK(c, wm_launch_bilinear(S0, S2, n, Hs[3], Ws[3], Hs[2], Ws[2], F_, nullptr, nullptr, c.s));
    float* cur = S2;  // output of the previous fusion block at level L
    // the two big resizes feed only a 3x3 conv: fuse them into that conv's input staging when the halo kernel applies
    const bool fuse_on = wm_tune(WM_TUNE_CONV_FUSE_UP, 1) != 0;
    const bool fuse_up1 = fuse_on && F_ % 64 == 0 && 4 * Hs[0] * Ws[0] >= 256;
    const bool fuse_up2 = fuse_on && !is_gs && (F_ / 2) % 64 == 0;
    // output_conv1 on the resized tensor as nine 1x1 products at the LOW resolution + a bilinear gather (upconv.hip): a quarter of the MFMA work
    const int Co1 = w.oc1.cout;
    const bool gather_on = wm_tune(WM_TUNE_UP1_GATHER, 1) != 0 && c.hdt == WM_DT_F16 && w.oc1_tap && F_ % 64 == 0 &&
                           w.oc1.cin == F_ && (Co1 == 128 || Co1 == 64 || Co1 == 32) &&
                           (unsigned long long)n * Hs[0] * Ws[0] * 9ull * (unsigned long long)Co1 * 2ull < (1ull << 32);   // the gather's 32-bit offsets
    bool up1_gather = false;
    const Up1Comp* comp = gather_on && wm_tune(WM_TUNE_UP1_COMP, 1) != 0 ? w.comp : nullptr;
    for (int L = 2; L >= 0; --L) {  // refinenet3 (level 2), refinenet2 (level 1), refinenet1 (level 0)
      float* others[3];
      others_than(hb.s, cur, others);
      // x = cur + RCU1(rn[L])
      st = rcu(c, w.rcu[L][0], rn[L], cur, others[0], others[1], n, Hs[L], Ws[L]);
      if (st) return st;
      // x = RCU2(x)
      st = rcu(c, w.rcu[L][1], others[1], nullptr, others[0], others[2], n, Hs[L], Ws[L], &x16);
      if (st) return st;
      const int Ho = L > 0 ? Hs[L - 1] : 2 * Hs[0], Wo = L > 0 ? Ws[L - 1] : 2 * Ws[0];
      up1_gather = L == 0 && gather_on && x16;
      if (up1_gather && comp != nullptr) { cur = others[2]; break; }   // out_conv lives inside the tap matrices: the tap GEMM reads x2 itself
      st = out_conv(c, w.out_conv[L], others[2], x16, others[0], n, Hs[L], Ws[L], F_, up1_gather);
      if (st) return st;
      if (L == 0 && (fuse_up1 || up1_gather)) { cur = others[0]; break; }  // the last resize is fused into output_conv1 (its input staging, or the tap form)
      LCHK(c, wm_launch_bilinear(others[0], others[1], n, Hs[L], Ws[L], Ho, Wo, F_, nullptr, nullptr, c.s));
      cur = others[1];
    }
    const int H8 = 8 * gh, W8 = 8 * gw;
    float* others[3];
    others_than(hb.s, cur, others);
    if (up1_gather) {
      void* Y1 = others[1];
      if (comp) st = gemm(c, c.hdt, WM_EPI_T16, cur, F_, comp->w16, F_, Y1, 9 * Co1, comp->bias, nullptr, n * Hs[0] * Ws[0], 9 * Co1, F_, nullptr, PK_OC1_UP);
      else st = gemm(c, c.hdt, WM_EPI_T16, cur, F_, w.oc1_tap, F_, Y1, 9 * Co1, nullptr, nullptr, n * Hs[0] * Ws[0], 9 * Co1, F_, nullptr, PK_OC1_UP);
      if (!st) {
        ProfScope ps(h, PK_OC1_UP, c.s);
        LCHK(c, wm_launch_upconv_gather(Y1, w.oc1.bias, others[0], n, Hs[0], Ws[0], H8, W8, Co1, c.s));
      }
    } else {
      WmConvArgs a = conv_args(cur, others[0], n, H8, W8, 3, 1, 1);
      if (fuse_up1) { a.up_hs = Hs[0]; a.up_ws = Ws[0]; }
      st = conv(c, w.oc1, a);
    }
    if (st) return st;
    const int Ho = gh * cf.patch_size, Wo = gw * cf.patch_size;
    float* fused = others[1];
    const float* posx = ws.posx[is_gs ? 1 : 0];
    const float* posy = ws.posy[is_gs ? 1 : 0];
    // output_conv2[0] un-fused (measured: 16-bit LDS-tiled resize 260 us + DMA-fed 32-channel conv 255 us vs 600-630 us for the
    // fused-resize kernel at 8 views, tools/bench_up_conv_n32.py): resize into `fused` as 16-bit, conv reads it by LDS-DMA
    bool tail_done = false;
    const bool up2_unfused = !is_gs && (F_ / 2) % 64 == 0 && F_ / 2 <= 128 && w.oc2_0.cout == 32;
    if (up2_unfused) {
      LCHK(c, wm_launch_bilinear16(others[0], fused, n, H8, W8, Ho, Wo, F_ / 2, posx, posy, c.hdt, c.s));
      WmConvN32Args a;
      memset(&a, 0, sizeof(a));
      a.x = (const uint16_t*)fused; a.w = (const uint16_t*)w.oc2_0.w16; a.bias = w.oc2_0.bias; a.y = others[2];
      a.zero = ws.ZERO256; a.N = n; a.H = Ho; a.W = Wo; a.Cin = F_ / 2; a.relu_out = 0; a.dtype = c.hdt;
      // ... with the head's tail (ReLU, 1x1 conv 32 -> C, activations) in its epilogue: the 32-channel tensor is never stored
      a.tail_w = w.oc2_2.w; a.tail_b = w.oc2_2.b; a.tail_C = out_dim; a.tail_act = act;
      a.tail_attr = out_attr + (size_t)v0 * Ho * Wo * (out_dim - 1); a.tail_conf = out_conf + (size_t)v0 * Ho * Wo;
      ProfScope ps(h, PK_OC2_TAIL, c.s);
      LCHK(c, wm_launch_conv3x3_n32_in16(a, c.s));
      tail_done = true;
    } else if (fuse_up2) {  // (the GS branch also needs the resized tensor itself: input_merger accumulates into it)
      WmConvArgs a = conv_args(others[0], others[2], n, Ho, Wo, 3, 1, 1);
      a.up_hs = H8; a.up_ws = W8; a.up_addx = posx; a.up_addy = posy;
      st = conv(c, w.oc2_0, a);
    } else {
      LCHK(c, wm_launch_bilinear(others[0], fused, n, H8, W8, Ho, Wo, F_ / 2, posx, posy, c.s));
      st = conv(c, w.oc2_0, conv_args(fused, others[2], n, Ho, Wo, 3, 1, 1));
    }
    if (st) return st;
    const size_t npix = (size_t)n * Ho * Wo, voff = (size_t)v0 * Ho * Wo;
    if (!tail_done)
      LCHK(c, wm_launch_dpt_tail(others[2], w.oc2_2.w, w.oc2_2.b, out_attr + voff * (out_dim - 1), out_conf + voff, npix, out_dim, act, c.s));
    if (is_gs && out->splat_means) {
      // dense_head.py:232-244: fused += ReLU(conv7x7(img)); then GaussianSplatRenderer.gs_head
      // (rasterization.py:149-153): conv3x3 (no bias) -> ReLU -> conv1x1 -> 12 raw parameters per pixel
      const float* img_c = img + (size_t)v0 * 3 * Ho * Wo;
      void* col = ws.gs_im2col;
      LCHK(c, wm_launch_im2col7(img_c, col, n, Ho, Wo, 192, c.hdt, c.s));
      WmGemmArgs ex;
      memset(&ex, 0, sizeof(ex));
      ex.rows_per_group = (int)npix; ex.accumulate = 1; ex.relu = 1;
      st = gemm(c, c.hdt, WM_EPI_ROWMAP_ADD, col, 192, w.merger.w, 192, fused, F_ / 2, w.merger.b, nullptr, (int)npix, F_ / 2, 192, &ex);
      if (st) return st;
      float* X = others[0];   // [n][H][W][gs_dim]
      float* gp = others[2];  // [n*H*W][12] (y32 is dead after the tail)
      st = conv(c, w.gs0, conv_args(fused, X, n, Ho, Wo, 3, 1, 1));
      if (st) return st;
      WmConvArgs a = conv_args(X, gp, n, Ho, Wo, 1, 1, 0);
      a.relu_in = 1;
      st = conv(c, w.gs2, a);
      if (st) return st;
      LCHK(c, wm_launch_gs_splat(gp, img_c, out_attr + voff, ws.cam_params + (size_t)(first_view + v0) * 9,
                                 out->splat_means + voff * 3, out->splat_quats + voff * 4, out->splat_scales + voff * 3,
                                 out->splat_opacities + voff, out->splat_sh + voff * 3, out->splat_weights + voff, n, Ho, Wo, c.s));
    }
  }
  return WM_OK;
}

}  // namespace wm_host
