// The planner: the arena layout for a shape, the binder that names every tensor and buffer for the last time, the host tables, and the
// queues and events the forward records and waits on.  Everything here runs from wm_reserve, never from the forward.
#include "wm_model.h"

namespace wm_host {

Dims make_dims(const wm_handle* h, int n, int nt, int H, int W) {
  const wm_config& c = h->cfg;
  Dims d;
  d.n = n; d.nt = nt; d.H = H; d.W = W;
  d.gh = H / c.patch_size; d.gw = W / c.patch_size; d.hw = d.gh * d.gw;
  d.R = c.num_register_tokens;
  d.Td = 1 + d.R + d.hw;
  d.psi = 1 + d.R + (c.enable_cond ? 2 : 0);
  d.P = d.psi + d.hw;
  d.D = c.embed_dim; d.heads = c.num_heads;
  d.Md = n * d.Td; d.Mv = n * d.P; d.Mx = std::max(d.Md, d.Mv);
  d.kpad_patch = ru(3 * c.patch_size * c.patch_size, 64);
  d.kpad_depth = ru(c.patch_size * c.patch_size, 64);
  d.world = nt / std::max(n, 1);
  d.chunk = std::min(n, 8);
  d.gh2 = (d.gh + 2 - 3) / 2 + 1; d.gw2 = (d.gw + 2 - 3) / 2 + 1;
  return d;
}

namespace {

// arena layout: name -> bytes (in a fixed order)
std::vector<std::pair<std::string, size_t>> arena_layout(const wm_handle* h, const Dims& d) {
  const wm_config& c = h->cfg;
  std::vector<std::pair<std::string, size_t>> L;
  auto add = [&](const char* n, size_t b) { L.push_back({n, (b + 255) / 256 * 256}); };
  const size_t D = d.D, Mx = d.Mx, Mv = d.Mv;
  add("Xd", (size_t)d.Md * D * 4);
  add("Xv", Mv * D * 4);
  add("A16", Mx * std::max<size_t>({D, (size_t)d.kpad_patch, (size_t)d.kpad_depth}) * 2);
  add("QKV16", 3 * Mx * D * 2);
  add("O16", Mx * D * 2);
  add("H16", Mx * 4 * D * 2);
  for (int i = 0; i < 4; ++i) add(("tap" + std::to_string(i)).c_str(), Mv * 2 * D * 4);
  add("KVG", (size_t)d.world * 2 * Mv * D * 2);
  add("ATT_PO", (size_t)WM_ATTN_MAX_SPLITS * Mx * D * 4);   // split-KV attention partials (tail round of a launch cut into up to 8 key slices; uniform 4-way split when a sharded launch fits one round): unnormalised O, (max, sum)
  add("ATT_ML", (size_t)WM_ATTN_MAX_SPLITS * Mx * (D / 64) * 2 * 4);
  add("ATT_FLAGS", wm_attention_max_blocks((int)Mx, d.P < d.Td ? d.P : d.Td, d.heads) * 4);  // per-block fallback flags of the no-max attention kernel
  // sticky fallback hints of the fast attention kernels (WmAttnArgs::unit_hint): one int per launch block, per attention call site
  // (DINO + frame + global blocks) x up to 3 launches (the piecewise form under the overlapped gather); zeroed by wm_reserve
  add("ATT_HINT", (size_t)(c.dino_depth + 2 * c.depth) * 3 * wm_attention_max_blocks((int)Mx, d.P < d.Td ? d.P : d.Td, d.heads) * 4);
  // fused LayerNorm of the residual GEMMs (WmGemmArgs::ln_out): per-row partials of the four column tiles, per-band arrival / departure
  // counters and fallback flags (zeroed by wm_reserve; the kernels leave the counters and flags at zero)
  add("LN_STATS", Mx * 4 * 2 * 4);
  add("LN_SYNC", (Mx / 16 + 2) * 3 * 4);
  add("ATT_STAT", (size_t)(c.dino_depth + 2 * c.depth) * 3 * 4);   // WmAttnArgs::unit_stat, one counter per (call site, launch)
  add("ZERO256", 256);  // zero page for the out-of-image halo pieces of the DMA-fed conv (conv_n32.hip); cleared at the start of every forward
  add("rope_cos", (size_t)(std::max(d.gh, d.gw) + 1) * 16 * 4);
  add("rope_sin", (size_t)(std::max(d.gh, d.gw) + 1) * 16 * 4);
  add("dino_pos", (size_t)(1 + d.hw) * D * 4);
  // priors
  add("pr_in", (size_t)d.n * 16 * 4);
  add("pr_h", (size_t)d.n * D * 4);
  add("pose_tok", (size_t)d.n * D * 4);
  add("ray_tok", (size_t)d.n * D * 4);
  // camera head (fp32, all views)
  const size_t D2 = 2 * D, nt = d.nt;
  add("cam_tok_local", (size_t)d.n * D2 * 4);
  add("cam_tok", nt * D2 * 4);
  add("cam_e", nt * D2 * 4);
  add("cam_mod", nt * 3 * D2 * 4);
  add("cam_h", nt * D2 * 4);
  add("cam_a", nt * D2 * 4);
  add("cam_qkv", nt * 3 * D2 * 4);
  add("cam_o", nt * D2 * 4);
  add("cam_f", nt * 4 * D2 * 4);
  add("cam_pred", nt * 12 * 4);
  add("cam_delta", nt * 12 * 4);
  add("cam_init", nt * 12 * 4);
  add("cam_params", nt * 9 * 4);
  // DPT heads
  const int32_t* oc = c.dpt_out_channels;
  const size_t ch = d.chunk, hw = d.hw;
  const int Fm = std::max(c.dpt_features, c.enable_gs ? c.gs_dim : 0);
  const int nslots = (c.enable_depth ? 1 : 0) + (c.enable_pts ? 1 : 0) + (c.enable_norm ? 1 : 0) + (c.enable_gs ? 1 : 0);
  const size_t big = ch * std::max<size_t>({64 * hw * (size_t)Fm, (size_t)d.H * d.W * (Fm / 2), (size_t)d.H * d.W * 32,
                                            c.enable_gs ? (size_t)d.H * d.W * c.gs_dim : 0}) * 4;
  // the shared tap front (tuning tap_shared) projects every tap of every view chunk before the heads fork: with two or more heads the four
  // projection outputs of a head hold all n views (dpt_P16b: the second tap's, which the direct form puts into dpt_P16 after the first's consumer)
  const size_t pv = nslots >= 2 ? (size_t)d.n : ch;
  for (int sl = 0; sl < std::max(nslots, 1); ++sl) {
    const std::string x = "_h" + std::to_string(sl);
    auto addh = [&](const char* n, size_t b) { add((std::string(n) + x).c_str(), b); };
    addh("dpt_T16", ch * hw * D2 * 2);   // (slot 0's is the shared front's normalised tap)
    addh("dpt_P16", pv * hw * std::max(oc[0], oc[1]) * 2);
    if (nslots >= 2) addh("dpt_P16b", pv * hw * oc[1] * 2);
    addh("dpt_f0", ch * 16 * hw * oc[0] * 4);
    addh("dpt_f1", ch * 4 * hw * oc[1] * 4);
    addh("dpt_f2", pv * hw * oc[2] * 4);
    addh("dpt_f3in", pv * hw * oc[3] * 4);
    addh("dpt_f3", ch * (size_t)d.gh2 * d.gw2 * oc[3] * 4);
    addh("dpt_rn1", ch * 16 * hw * Fm * 4);
    addh("dpt_rn2", ch * 4 * hw * Fm * 4);
    addh("dpt_rn3", ch * hw * Fm * 4);
    addh("dpt_rn4", ch * (size_t)d.gh2 * d.gw2 * Fm * 4);
    for (int i = 0; i < 4; ++i) addh(("dpt_s" + std::to_string(i)).c_str(), big);
  }
  if (c.enable_gs) add("gs_im2col", ch * (size_t)d.H * d.W * 192 * 2);
  for (int i = 0; i < 4; ++i) add(("dpt_pos" + std::to_string(i)).c_str(), hw * oc[i] * 4);
  add("dpt_posx", (size_t)d.W * (Fm / 4) * 4 * 2);  // one table per feature width (F/2 channels -> F/4 per axis)
  add("dpt_posy", (size_t)d.H * (Fm / 4) * 4 * 2);
  add("gs_posx", (size_t)d.W * (Fm / 4) * 4 * 2);
  add("gs_posy", (size_t)d.H * (Fm / 4) * 4 * 2);
  return L;
}

// torch.linspace(start, end, steps, dtype=float32) (symmetric evaluation, as ATen does)
void linspace_f32(float start, float end, int steps, std::vector<float>& out) {
  out.resize(steps);
  if (steps == 1) { out[0] = start; return; }
  const float step = (end - start) / (float)(steps - 1);
  const int half = steps / 2;
  for (int i = 0; i < steps; ++i) out[i] = i < half ? start + step * (float)i : end - step * (float)(steps - i - 1);
}

// src/models/utils/grid.py:4-90 — separable halves of 0.1 * position_grid_to_embed(create_uv_grid(w,h,aspect), C)
void uv_tables(int w, int hgt, int C, double aspect, std::vector<float>& tx, std::vector<float>& ty) {
  const double diag = std::sqrt(aspect * aspect + 1.0), sx = aspect / diag, sy = 1.0 / diag;
  std::vector<float> u, v;
  linspace_f32((float)(-sx * (w - 1) / w), (float)(sx * (w - 1) / w), w, u);
  linspace_f32((float)(-sy * (hgt - 1) / hgt), (float)(sy * (hgt - 1) / hgt), hgt, v);
  const int q = C / 4;
  std::vector<double> om(q);
  for (int k = 0; k < q; ++k) om[k] = 1.0 / std::pow(100.0, (double)k / (C / 4.0));
  tx.assign((size_t)w * 2 * q, 0.f);
  ty.assign((size_t)hgt * 2 * q, 0.f);
  for (int x = 0; x < w; ++x)
    for (int k = 0; k < q; ++k) {
      tx[(size_t)x * 2 * q + k] = (float)std::sin((double)u[x] * om[k]) * 0.1f;
      tx[(size_t)x * 2 * q + q + k] = (float)std::cos((double)u[x] * om[k]) * 0.1f;
    }
  for (int y = 0; y < hgt; ++y)
    for (int k = 0; k < q; ++k) {
      ty[(size_t)y * 2 * q + k] = (float)std::sin((double)v[y] * om[k]) * 0.1f;
      ty[(size_t)y * 2 * q + q + k] = (float)std::cos((double)v[y] * om[k]) * 0.1f;
    }
}

// ATen's separable anti-aliased bicubic (a = -0.5), align_corners=False — vision_transformer.py:196-201
inline double cubic_aa(double x) {
  const double a = -0.5;
  x = std::fabs(x);
  if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1.0;
  if (x < 2.0) return (((x - 5.0) * x + 8.0) * x - 4.0) * a;
  return 0.0;
}
void aa_weights(int in, int out, std::vector<int>& xmin, std::vector<int>& xsize, std::vector<float>& wts, int& maxk) {
  const double scale = (double)in / out;
  const double support = scale >= 1.0 ? 2.0 * scale : 2.0;
  const double invscale = scale >= 1.0 ? 1.0 / scale : 1.0;
  maxk = (int)std::ceil(support) * 2 + 1;
  xmin.resize(out); xsize.resize(out); wts.assign((size_t)out * maxk, 0.f);
  for (int i = 0; i < out; ++i) {
    const double center = scale * (i + 0.5);
    const int lo = std::max(0, (int)(center - support + 0.5));
    const int hi = std::min(in, (int)(center + support + 0.5));
    xmin[i] = lo; xsize[i] = hi - lo;
    double tot = 0;
    std::vector<double> w(hi - lo);
    for (int j = 0; j < hi - lo; ++j) { w[j] = cubic_aa((j + lo - center + 0.5) * invscale); tot += w[j]; }
    for (int j = 0; j < hi - lo; ++j) wts[(size_t)i * maxk + j] = (float)(w[j] / tot);
  }
}

}  // namespace
}  // namespace wm_host
using namespace wm_host;

extern "C" void wm_host_resample_pos(const float* in, int gs, int D, int gh, int gw, float* out) {
  // in [gs][gs][D] -> out [gh][gw][D]; horizontal pass then vertical pass (ATen order)
  std::vector<int> xm, xs, ym, ys;
  std::vector<float> xw, yw;
  int kx, ky;
  aa_weights(gs, gw, xm, xs, xw, kx);
  aa_weights(gs, gh, ym, ys, yw, ky);
  std::vector<float> tmp((size_t)gs * gw * D);
  for (int y = 0; y < gs; ++y)
    for (int x = 0; x < gw; ++x) {
      float* o = &tmp[((size_t)y * gw + x) * D];
      for (int c = 0; c < D; ++c) o[c] = 0.f;
      for (int j = 0; j < xs[x]; ++j) {
        const float w = xw[(size_t)x * kx + j];
        const float* s = in + ((size_t)y * gs + xm[x] + j) * D;
        for (int c = 0; c < D; ++c) o[c] += w * s[c];
      }
    }
  for (int y = 0; y < gh; ++y)
    for (int x = 0; x < gw; ++x) {
      float* o = out + ((size_t)y * gw + x) * D;
      for (int c = 0; c < D; ++c) o[c] = 0.f;
      for (int j = 0; j < ys[y]; ++j) {
        const float w = yw[(size_t)y * ky + j];
        const float* s = &tmp[((size_t)(ym[y] + j) * gw + x) * D];
        for (int c = 0; c < D; ++c) o[c] += w * s[c];
      }
    }
}

namespace wm_host {
namespace {

// The one place where a tensor or a workspace buffer is addressed by name.  Every name goes through Binder: an absent name, or a tensor
// without the form the forward needs (fp32 / 16-bit repack), is remembered (the first one) and fails wm_reserve with that name.
struct Binder {
  const wm_handle* h;
  const std::map<std::string, char*>& buf;
  std::string err;
  void miss(const std::string& what) { if (err.empty()) err = what; }
  const Weight* tensor(const std::string& n) {
    const Weight* w = W(h, n);
    if (!w) miss("no tensor " + n);
    return w;
  }
  const float* f32(const std::string& n) {
    const Weight* w = tensor(n);
    if (w && !w->f32) miss(n + " has no fp32 form");
    return w ? w->f32 : nullptr;
  }
  const void* w16(const std::string& n) {
    const Weight* w = tensor(n);
    if (w && !w->w16) miss(n + " has no 16-bit form");
    return w ? w->w16 : nullptr;
  }
  Norm norm(const std::string& p) { return {f32(p + ".weight"), f32(p + ".bias")}; }
  Lin16 lin16(const std::string& p) { return {w16(p + ".weight"), f32(p + ".bias")}; }
  Lin32 lin32(const std::string& p) {   // N and K from the shape: [N][K...]
    Lin32 l;
    l.w = f32(p + ".weight"); l.b = f32(p + ".bias");
    const Weight* w = tensor(p + ".weight");
    if (w && !w->shape.empty()) {
      l.N = (int)w->shape[0]; l.K = 1;
      for (size_t i = 1; i < w->shape.size(); ++i) l.K *= (int)w->shape[i];
    }
    return l;
  }
  ConvW conv(const std::string& p, bool bias = true) {   // [Cout][Cin][k][k]
    ConvW cv;
    cv.w16 = w16(p + ".weight");
    const Weight* w = tensor(p + ".weight");
    if (w && w->shape.size() == 4) { cv.cout = (int)w->shape[0]; cv.cin = (int)w->shape[1]; }
    else if (w) miss(p + ".weight is not a conv weight");
    if (bias) cv.bias = f32(p + ".bias");
    return cv;
  }
  template <class T> T* ws(const std::string& n) {
    auto it = buf.find(n);
    if (it == buf.end()) { miss("no workspace buffer " + n); return nullptr; }
    return (T*)it->second;
  }
};

// Fills h->m and h->ws from the finalized weights, the composed head weights (tconv / up1comp) and the arena's buffer map
wm_status bind_model(wm_handle* h, const std::map<std::string, char*>& buf) {
  const wm_config& c = h->cfg;
  Binder b{h, buf, std::string()};
  Model m;
  Workspace w;
  const std::string v = "visual_geometry_transformer.", dn = v + "patch_embed.", ch = "cam_head.";
  auto block = [&](const std::string& p, bool qk_norm) {
    BlockW k;
    k.norm1 = b.norm(p + "norm1"); k.norm2 = b.norm(p + "norm2");
    k.qkv = b.lin16(p + "attn.qkv"); k.proj = b.lin16(p + "attn.proj"); k.fc1 = b.lin16(p + "mlp.fc1"); k.fc2 = b.lin16(p + "mlp.fc2");
    if (qk_norm) { k.q_norm = b.norm(p + "attn.q_norm"); k.k_norm = b.norm(p + "attn.k_norm"); }   // optional: the DINO blocks have no q/k-norm
    k.ls1 = b.f32(p + "ls1.gamma"); k.ls2 = b.f32(p + "ls2.gamma");
    return k;
  };
  m.patch_proj = b.lin16(dn + "patch_embed.proj");
  m.cls_token = b.f32(dn + "cls_token"); m.register_tokens = b.f32(dn + "register_tokens");
  m.cam_token = b.f32(v + "cam_token"); m.reg_token = b.f32(v + "reg_token");
  m.dino_norm = b.norm(dn + "norm");
  for (int i = 0; i < c.dino_depth; ++i) m.dino.push_back(block(dn + "blocks." + std::to_string(i) + ".", false));
  for (int i = 0; i < c.depth; ++i) {
    m.frame.push_back(block(v + "frame_blocks." + std::to_string(i) + ".", true));
    m.global.push_back(block(v + "global_blocks." + std::to_string(i) + ".", true));
  }
  if (c.enable_cond) {
    m.pose_embed[0] = b.lin32(v + "pose_embed.0"); m.pose_embed[1] = b.lin32(v + "pose_embed.2");
    m.ray_embed[0] = b.lin32(v + "ray_embed.0"); m.ray_embed[1] = b.lin32(v + "ray_embed.2");
    m.depth_fc1 = b.lin16(v + "depth_embed.proj.2.fc1"); m.depth_fc2 = b.lin16(v + "depth_embed.proj.2.fc2");
  }
  if (c.enable_cam) {
    m.cam_token_norm = b.norm(ch + "token_norm"); m.cam_out_norm = b.norm(ch + "out_norm");
    m.cam_param_embed = b.lin32(ch + "param_embed"); m.cam_adapt = b.lin32(ch + "adapt_norm_gen.1");
    m.cam_pred_fc1 = b.lin32(ch + "param_predictor.fc1"); m.cam_pred_fc2 = b.lin32(ch + "param_predictor.fc2");
    for (int i = 0; i < c.cam_trunk_depth; ++i) {
      const std::string p = ch + "refine_net." + std::to_string(i) + ".";
      CamBlockW k;
      k.norm1 = b.norm(p + "norm1"); k.norm2 = b.norm(p + "norm2");
      k.qkv = b.lin32(p + "attn.qkv"); k.proj = b.lin32(p + "attn.proj"); k.fc1 = b.lin32(p + "mlp.fc1"); k.fc2 = b.lin32(p + "mlp.fc2");
      k.ls1 = b.f32(p + "ls1.gamma"); k.ls2 = b.f32(p + "ls2.gamma");
      m.cam.push_back(k);
    }
  }
  for (int id = 0; id < HD_COUNT; ++id) {
    if (!head_enabled(c, id)) continue;
    const std::string p = kHeadPrefix[id], sc = p + "scratch.";
    const int F_ = id == HD_GS ? c.gs_dim : c.dpt_features;
    HeadW& hw = m.head[id];
    hw.norm = b.norm(p + "norm");
    for (int i = 0; i < 4; ++i) hw.proj[i] = b.lin16(p + "projects." + std::to_string(i));
    for (int i = 0; i < 2; ++i) hw.resize[i] = b.lin16(p + "resize_layers." + std::to_string(i));
    hw.resize3 = b.conv(p + "resize_layers.3");
    for (int i = 0; i < 4; ++i) hw.rn[i] = b.conv(sc + "layer" + std::to_string(i + 1) + "_rn", false);   // optional: Conv2d(bias=False)
    for (int r = 1; r <= 4; ++r) {
      const std::string q = sc + "refinenet" + std::to_string(r) + ".";
      hw.out_conv[r - 1] = b.conv(q + "out_conv");
      if (hw.out_conv[r - 1].cin != F_ || hw.out_conv[r - 1].cout != F_) b.miss(q + "out_conv.weight is not [F][F][1][1]");
      for (int u = (r == 4 ? 2 : 1); u <= 2; ++u)
        for (int cv = 1; cv <= 2; ++cv) hw.rcu[r - 1][u - 1][cv - 1] = b.conv(q + "resConfUnit" + std::to_string(u) + ".conv" + std::to_string(cv));
    }
    hw.oc1 = b.conv(sc + "output_conv1");
    const Weight* w1 = b.tensor(sc + "output_conv1.weight");
    if (w1 && w1->w16 && w1->tap_major) hw.oc1_tap = (const uint16_t*)w1->w16 + (size_t)hw.oc1.cout * 9 * hw.oc1.cin;   // optional: 3x3 weights only
    const Up1Comp& u1 = h->up1comp[id];
    hw.comp = u1.w16 && u1.co == hw.oc1.cout ? &u1 : nullptr;                            // optional: f16 heads of the dense kind only
    hw.oc2_0 = b.conv(sc + "output_conv2.0");
    hw.oc2_2 = b.lin32(sc + "output_conv2.2");
    if (id == HD_GS) {
      hw.merger = b.lin16(p + "input_merger.0");
      hw.gs0 = b.conv("gs_renderer.gs_head.0", false);                                   // optional: Conv2d(bias=False)
      hw.gs2 = b.conv("gs_renderer.gs_head.2");
    }
    for (int i = 0; i < 2; ++i) hw.tconv[i] = h->tconv[id][i].w16 ? &h->tconv[id][i] : nullptr;   // optional: 256-feature dense heads only
  }

  w.Xd = b.ws<float>("Xd"); w.Xv = b.ws<float>("Xv"); w.A16 = b.ws<uint16_t>("A16"); w.QKV16 = b.ws<char>("QKV16");
  w.O16 = b.ws<void>("O16"); w.H16 = b.ws<void>("H16"); w.KVG = b.ws<char>("KVG");
  for (int i = 0; i < 4; ++i) w.tap[i] = b.ws<float>("tap" + std::to_string(i));
  w.ATT_PO = b.ws<float>("ATT_PO"); w.ATT_ML = b.ws<float>("ATT_ML"); w.ATT_FLAGS = b.ws<int>("ATT_FLAGS"); w.ATT_HINT = b.ws<int>("ATT_HINT");
  w.ATT_STAT = b.ws<int>("ATT_STAT"); w.LN_STATS = b.ws<float>("LN_STATS"); w.LN_SYNC = b.ws<int>("LN_SYNC"); w.ZERO256 = b.ws<uint16_t>("ZERO256");
  w.rope_cos = b.ws<float>("rope_cos"); w.rope_sin = b.ws<float>("rope_sin"); w.dino_pos = b.ws<float>("dino_pos");
  w.pr_in = b.ws<float>("pr_in"); w.pr_h = b.ws<float>("pr_h"); w.pose_tok = b.ws<float>("pose_tok"); w.ray_tok = b.ws<float>("ray_tok");
  w.cam_tok_local = b.ws<float>("cam_tok_local"); w.cam_tok = b.ws<float>("cam_tok"); w.cam_e = b.ws<float>("cam_e"); w.cam_mod = b.ws<float>("cam_mod");
  w.cam_h = b.ws<float>("cam_h"); w.cam_a = b.ws<float>("cam_a"); w.cam_qkv = b.ws<float>("cam_qkv"); w.cam_o = b.ws<float>("cam_o");
  w.cam_f = b.ws<float>("cam_f"); w.cam_pred = b.ws<float>("cam_pred"); w.cam_delta = b.ws<float>("cam_delta"); w.cam_init = b.ws<float>("cam_init");
  w.cam_params = b.ws<float>("cam_params");
  int nslots = 0;
  for (int id = 0; id < HD_COUNT; ++id) nslots += head_enabled(c, id) ? 1 : 0;
  for (int sl = 0; sl < std::max(nslots, 1); ++sl) {
    const std::string x = "_h" + std::to_string(sl);
    HeadBufs& q = w.hb[sl];
    q.T16 = b.ws<void>("dpt_T16" + x); q.P16 = b.ws<void>("dpt_P16" + x);
    if (nslots >= 2) q.P16b = b.ws<void>("dpt_P16b" + x);   // optional: laid out for the shared tap front only
    q.f0 = b.ws<float>("dpt_f0" + x); q.f1 = b.ws<float>("dpt_f1" + x); q.f2 = b.ws<float>("dpt_f2" + x); q.f3in = b.ws<float>("dpt_f3in" + x);
    q.f3 = b.ws<float>("dpt_f3" + x);
    for (int i = 0; i < 4; ++i) {
      q.rn[i] = b.ws<float>("dpt_rn" + std::to_string(i + 1) + x);
      q.s[i] = b.ws<float>("dpt_s" + std::to_string(i) + x);
    }
  }
  if (c.enable_gs) w.gs_im2col = b.ws<void>("gs_im2col");
  for (int i = 0; i < 4; ++i) w.dpt_pos[i] = b.ws<float>("dpt_pos" + std::to_string(i));
  w.posx[0] = b.ws<float>("dpt_posx"); w.posy[0] = b.ws<float>("dpt_posy"); w.posx[1] = b.ws<float>("gs_posx"); w.posy[1] = b.ws<float>("gs_posy");
  if (!b.err.empty()) return fail(h, WM_ERR_STATE, "wm_reserve: " + b.err);
  h->m = std::move(m);
  h->ws = w;
  return WM_OK;
}

// The queues and events on which the forward forks the camera head and the DPT heads: once per handle, kept across re-plans, destroyed by
// wm_destroy.  Whatever the tuning says now (it may change after the reserve); in the order the forward first uses them.
wm_status create_head_queues(wm_handle* h) {
  const wm_config& c = h->cfg;
  if (!h->hfork) HIPCHK(h, hipEventCreateWithFlags(&h->hfork, hipEventDisableTiming));
  if (c.enable_cam) {
    if (!h->camstream) HIPCHK(h, hipStreamCreateWithFlags(&h->camstream, hipStreamNonBlocking));
    if (!h->camjoin) HIPCHK(h, hipEventCreateWithFlags(&h->camjoin, hipEventDisableTiming));
  }
  if (!h->hfront) HIPCHK(h, hipEventCreateWithFlags(&h->hfront, hipEventDisableTiming));
  int nheads = 0;
  for (int id = 0; id < HD_COUNT; ++id) nheads += head_enabled(c, id) ? 1 : 0;
  for (int k = 0; k < nheads; ++k) {
    if (!h->hstream[k]) HIPCHK(h, hipStreamCreateWithFlags(&h->hstream[k], hipStreamNonBlocking));
    if (!h->hjoin[k]) HIPCHK(h, hipEventCreateWithFlags(&h->hjoin[k], hipEventDisableTiming));
  }
  return WM_OK;
}

// Builds the workspace for a shape: arena (library-owned unless the caller gave one), the composed head weights, the bound model
// (bind_model), the shape- / weight-derived device tables and the heads' queues.  Called by wm_reserve only — never from the forward pass.
wm_status plan(wm_handle* h, const Dims& d) {
  if (h->plan_n == d.n && h->plan_nt == d.nt && h->plan_H == d.H && h->plan_W == d.W) return WM_OK;
  h->plan_n = -1;   // until this plan is complete the forward has nothing to run on
  const wm_config& c = h->cfg;
  auto L = arena_layout(h, d);
  size_t tot = 0;
  for (auto& kv : L) tot += kv.second;
  HIPCHK(h, hipDeviceSynchronize());  // a forward of the previous shape may still be using the arena
  if (tot > h->arena_bytes) {
    if (!h->arena_owned)
      return fail(h, WM_ERR_STATE, "caller workspace too small: " + std::to_string(h->arena_bytes) + " < " + std::to_string(tot) + " bytes (wm_workspace_bytes)");
    if (h->arena) HIPCHK(h, hipFree(h->arena));
    h->arena = nullptr;
    h->arena_bytes = 0;
    HIPCHK(h, hipMalloc((void**)&h->arena, tot));
    h->arena_bytes = tot;
  }
  std::map<std::string, char*> buf;
  size_t off = 0;
  for (auto& kv : L) { buf[kv.first] = h->arena + off; off += kv.second; }

  {
    const wm_status st = rebuild_weight_derived(h, d);
    if (st != WM_OK) return st;
  }
  // every weight and workspace buffer the forward reads, by name for the last time
  {
    const wm_status st = bind_model(h, buf);
    if (st != WM_OK) return st;
  }
  const Workspace& ws = h->ws;

  // RoPE tables (rope.py:80-111): angle = pos * 100^(-i/16), i < 16 (table is cat(ang, ang): index e % 16)
  {
    const int np = std::max(d.gh, d.gw) + 1;
    std::vector<float> cs((size_t)np * 16), sn((size_t)np * 16);
    for (int p = 0; p < np; ++p)
      for (int i = 0; i < 16; ++i) {
        const float expo = (float)(2 * i) / 32.0f;
        const float inv = 1.0f / std::pow(c.rope_freq, expo);
        const float ang = (float)p * inv;
        cs[(size_t)p * 16 + i] = std::cos(ang);
        sn[(size_t)p * 16 + i] = std::sin(ang);
      }
    HIPCHK(h, hipMemcpy(ws.rope_cos, cs.data(), cs.size() * 4, hipMemcpyHostToDevice));
    HIPCHK(h, hipMemcpy(ws.rope_sin, sn.data(), sn.size() * 4, hipMemcpyHostToDevice));
  }
  {  // fallback statistics: counters at 0, host mirror allocated once (pinned: the forward copies into it without synchronising)
    const int n = (c.dino_depth + 2 * c.depth) * 3;
    if (h->att_stat_n != n) {
      if (h->att_stat_host) HIPCHK(h, hipHostFree(h->att_stat_host));
      h->att_stat_host = nullptr;
      HIPCHK(h, hipHostMalloc((void**)&h->att_stat_host, (size_t)n * 4, hipHostMallocDefault));
      h->att_stat_n = n;
    }
    memset(h->att_stat_host, 0, (size_t)n * 4);
    h->att_seen.assign(n, 0);
    h->att_general_ttl.assign(n, 0);
    HIPCHK(h, hipMemset(ws.ATT_STAT, 0, (size_t)n * 4));
  }
  HIPCHK(h, hipMemset(ws.LN_SYNC, 0, ((size_t)d.Mx / 16 + 2) * 3 * 4));
  // the fast attention kernels' sticky fallback hints start empty for a new shape (they index launch blocks)
  HIPCHK(h, hipMemset(ws.ATT_HINT, 0, (size_t)(c.dino_depth + 2 * c.depth) * 3 * wm_attention_max_blocks((int)d.Mx, d.P < d.Td ? d.P : d.Td, d.heads) * 4));
  // DINO pos-embed for this grid (vision_transformer.py:175-207)
  {
    const Weight* pe = W(h, "visual_geometry_transformer.patch_embed.pos_embed");
    if (!pe || pe->host.empty()) return fail(h, WM_ERR_STATE, "pos_embed not set");
    const int g = c.img_size / c.patch_size, D = d.D;
    if (d.gh == g && d.gw == g) {
      HIPCHK(h, hipMemcpy(ws.dino_pos, pe->host.data(), (size_t)(1 + d.hw) * D * 4, hipMemcpyHostToDevice));
    } else {
      std::vector<float> r((size_t)(1 + d.hw) * D);
      memcpy(r.data(), pe->host.data(), (size_t)D * 4);
      wm_host_resample_pos(pe->host.data() + D, g, D, d.gh, d.gw, r.data() + D);
      HIPCHK(h, hipMemcpy(ws.dino_pos, r.data(), r.size() * 4, hipMemcpyHostToDevice));
    }
  }
  // DPT UV position tables (dense_head.py:253-263)
  {
    const double aspect = (double)d.W / (double)d.H;
    std::vector<float> tx, ty;
    for (int i = 0; i < 4; ++i) {
      const int C = c.dpt_out_channels[i];
      uv_tables(d.gw, d.gh, C, aspect, tx, ty);
      std::vector<float> full((size_t)d.hw * C);
      for (int y = 0; y < d.gh; ++y)
        for (int x = 0; x < d.gw; ++x)
          for (int k = 0; k < C; ++k)
            full[((size_t)y * d.gw + x) * C + k] = k < C / 2 ? tx[(size_t)x * (C / 2) + k] : ty[(size_t)y * (C / 2) + k - C / 2];
      HIPCHK(h, hipMemcpy(ws.dpt_pos[i], full.data(), full.size() * 4, hipMemcpyHostToDevice));
    }
    uv_tables(d.W, d.H, c.dpt_features / 2, aspect, tx, ty);
    HIPCHK(h, hipMemcpy(ws.posx[0], tx.data(), tx.size() * 4, hipMemcpyHostToDevice));
    HIPCHK(h, hipMemcpy(ws.posy[0], ty.data(), ty.size() * 4, hipMemcpyHostToDevice));
    if (c.enable_gs) {
      uv_tables(d.W, d.H, c.gs_dim / 2, aspect, tx, ty);
      HIPCHK(h, hipMemcpy(ws.posx[1], tx.data(), tx.size() * 4, hipMemcpyHostToDevice));
      HIPCHK(h, hipMemcpy(ws.posy[1], ty.data(), ty.size() * 4, hipMemcpyHostToDevice));
    }
  }
  // camera init token broadcast [nt][12]
  if (c.enable_cam) {
    const Weight* it = W(h, "cam_head.init_token");
    std::vector<float> v((size_t)d.nt * 12, 0.f);
    if (it && !it->host.empty())
      for (int i = 0; i < d.nt; ++i)
        for (int k = 0; k < 9; ++k) v[(size_t)i * 12 + k] = it->host[k];
    HIPCHK(h, hipMemcpy(ws.cam_init, v.data(), v.size() * 4, hipMemcpyHostToDevice));
  }
  {
    const wm_status st = create_head_queues(h);
    if (st != WM_OK) return st;
  }
  h->plan_n = d.n; h->plan_nt = d.nt; h->plan_H = d.H; h->plan_W = d.W;
  return WM_OK;
}

}  // namespace
}  // namespace wm_host

// ====================================================================================== workspace
extern "C" size_t wm_workspace_bytes(const wm_handle* h, int n_local, int n_total, int H, int W) {
  if (!h) return 0;
  const Dims d = make_dims(h, n_local, n_total, H, W);
  size_t tot = 0;
  for (auto& kv : arena_layout(h, d)) tot += kv.second;
  return tot;
}

extern "C" wm_status wm_set_workspace(wm_handle* h, void* device_ptr, size_t bytes) {
  if (!h) return WM_ERR_INVALID;
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipDeviceSynchronize());
  if (h->arena && h->arena_owned) HIPCHK(h, hipFree(h->arena));
  h->arena = (char*)device_ptr;
  h->arena_bytes = device_ptr ? bytes : 0;
  h->arena_owned = device_ptr == nullptr;  // NULL hands the arena back to the library
  h->plan_n = -1;   // (the bound workspace pointers go with the plan)
  return WM_OK;
}

extern "C" wm_status wm_reserve(wm_handle* h, int n_local, int n_total, int H, int W) {
  if (!h) return WM_ERR_INVALID;
  if (!h->finalized) return fail(h, WM_ERR_STATE, "weights not finalized");
  if (n_local <= 0 || n_total < n_local || n_total % n_local) return fail(h, WM_ERR_INVALID, "n_total must be a positive multiple of n_local");
  if (H <= 0 || W <= 0 || H % h->cfg.patch_size || W % h->cfg.patch_size) return fail(h, WM_ERR_INVALID, "H and W must be multiples of patch_size");
  HIPCHK(h, hipSetDevice(h->device));
  return plan(h, make_dims(h, n_local, n_total, H, W));
}
