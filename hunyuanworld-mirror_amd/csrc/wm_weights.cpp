// The weight store of a handle: the parameter list, the 16-bit repack at load, and the handle's lifecycle.
#include "wm_model.h"

namespace wm_host {
namespace {

// ------------------------------------------------------------------ host 16-bit conversion
inline uint16_t h_f2bf(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);  // NaN stays NaN
  return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}
inline uint16_t h_f2h(float f) {
  _Float16 h = (_Float16)f;
  uint16_t r;
  memcpy(&r, &h, 2);
  return r;
}

bool ends_with(const std::string& s, const char* suf) {
  const size_t n = strlen(suf);
  return s.size() >= n && s.compare(s.size() - n, n, suf) == 0;
}
bool starts_with(const std::string& s, const char* p) { return s.compare(0, strlen(p), p) == 0; }
// the tensors build_tapfold composes (kept in fp32 on the host): a DPT head's norm.{weight,bias} and projects.i.{weight,bias}
bool is_tapfold_source(const std::string& n) {
  for (const char* p : kHeadPrefix)
    if (starts_with(n, p)) {
      const std::string r = n.substr(strlen(p));
      return r == "norm.weight" || r == "norm.bias" || starts_with(r, "projects.");
    }
  return false;
}

enum WKind { WK_F32, WK_LIN16_BACKBONE, WK_LIN16_HEAD, WK_CONV16_HEAD, WK_CONVT16_HEAD };

WKind classify(const std::string& n, int ndim) {
  const bool vgt = starts_with(n, "visual_geometry_transformer.");
  if (vgt && ndim >= 2) {
    if (ends_with(n, "attn.qkv.weight") || ends_with(n, "attn.proj.weight") || ends_with(n, "mlp.fc1.weight") ||
        ends_with(n, "mlp.fc2.weight") || ends_with(n, "patch_embed.proj.weight") || ends_with(n, "depth_embed.proj.2.fc1.weight") ||
        ends_with(n, "depth_embed.proj.2.fc2.weight"))
      return WK_LIN16_BACKBONE;
    return WK_F32;
  }
  const bool head = std::any_of(std::begin(kHeadPrefix), std::end(kHeadPrefix), [&](const char* p) { return starts_with(n, p); });
  if (head && ndim == 4 && ends_with(n, ".weight")) {
    if (ends_with(n, "scratch.output_conv2.2.weight")) return WK_F32;
    if (n.find("input_merger") != std::string::npos) return WK_LIN16_HEAD;  // 7x7 conv on the image as a GEMM, K = 3*49
    if (n.find("resize_layers.0.") != std::string::npos || n.find("resize_layers.1.") != std::string::npos) return WK_CONVT16_HEAD;
    if (n.find(".projects.") != std::string::npos) return WK_LIN16_HEAD;
    return WK_CONV16_HEAD;
  }
  if (n == "gs_renderer.gs_head.0.weight" || n == "gs_renderer.gs_head.2.weight") return WK_CONV16_HEAD;
  return WK_F32;
}

// ------------------------------------------------------------------ parameter list (mirrors config.param_spec)
void spec_block(std::vector<std::pair<std::string, std::vector<int64_t>>>& s, const std::string& p, int D, int hid, int qk) {
  auto add = [&](const char* n, std::vector<int64_t> sh) { s.push_back({p + n, sh}); };
  add("norm1.weight", {D}); add("norm1.bias", {D});
  add("attn.qkv.weight", {3 * D, D}); add("attn.qkv.bias", {3 * D});
  if (qk) { add("attn.q_norm.weight", {qk}); add("attn.q_norm.bias", {qk}); add("attn.k_norm.weight", {qk}); add("attn.k_norm.bias", {qk}); }
  add("attn.proj.weight", {D, D}); add("attn.proj.bias", {D}); add("ls1.gamma", {D});
  add("norm2.weight", {D}); add("norm2.bias", {D});
  add("mlp.fc1.weight", {hid, D}); add("mlp.fc1.bias", {hid}); add("mlp.fc2.weight", {D, hid}); add("mlp.fc2.bias", {D});
  add("ls2.gamma", {D});
}

std::vector<std::pair<std::string, std::vector<int64_t>>> param_spec(const wm_config& c) {
  std::vector<std::pair<std::string, std::vector<int64_t>>> s;
  const int D = c.embed_dim, g = c.img_size / c.patch_size, R = c.num_register_tokens, H4 = c.mlp_ratio * D;
  const std::string v = "visual_geometry_transformer.", d = v + "patch_embed.";
  s.push_back({v + "cam_token", {1, 2, 1, D}});
  s.push_back({v + "reg_token", {1, 2, R, D}});
  s.push_back({d + "cls_token", {1, 1, D}});
  s.push_back({d + "pos_embed", {1, 1 + g * g, D}});
  s.push_back({d + "register_tokens", {1, R, D}});
  s.push_back({d + "patch_embed.proj.weight", {D, 3, c.patch_size, c.patch_size}});
  s.push_back({d + "patch_embed.proj.bias", {D}});
  for (int i = 0; i < c.dino_depth; ++i) spec_block(s, d + "blocks." + std::to_string(i) + ".", D, H4, 0);
  s.push_back({d + "norm.weight", {D}});
  s.push_back({d + "norm.bias", {D}});
  if (c.enable_cond) {
    s.push_back({v + "pose_embed.0.weight", {D, 7}}); s.push_back({v + "pose_embed.0.bias", {D}});
    s.push_back({v + "pose_embed.2.weight", {D, D}}); s.push_back({v + "pose_embed.2.bias", {D}});
    s.push_back({v + "depth_embed.proj.2.fc1.weight", {4 * D, c.patch_size * c.patch_size}});
    s.push_back({v + "depth_embed.proj.2.fc1.bias", {4 * D}});
    s.push_back({v + "depth_embed.proj.2.fc2.weight", {D, 4 * D}}); s.push_back({v + "depth_embed.proj.2.fc2.bias", {D}});
    s.push_back({v + "ray_embed.0.weight", {D, 4}}); s.push_back({v + "ray_embed.0.bias", {D}});
    s.push_back({v + "ray_embed.2.weight", {D, D}}); s.push_back({v + "ray_embed.2.bias", {D}});
  }
  for (int i = 0; i < c.depth; ++i) spec_block(s, v + "frame_blocks." + std::to_string(i) + ".", D, H4, D / c.num_heads);
  for (int i = 0; i < c.depth; ++i) spec_block(s, v + "global_blocks." + std::to_string(i) + ".", D, H4, D / c.num_heads);
  const int D2 = 2 * D;
  if (c.enable_cam) {
    const std::string ch = "cam_head.";
    for (int i = 0; i < c.cam_trunk_depth; ++i) spec_block(s, ch + "refine_net." + std::to_string(i) + ".", D2, 4 * D2, 0);
    s.push_back({ch + "token_norm.weight", {D2}}); s.push_back({ch + "token_norm.bias", {D2}});
    s.push_back({ch + "out_norm.weight", {D2}}); s.push_back({ch + "out_norm.bias", {D2}});
    s.push_back({ch + "init_token", {1, 1, 9}});
    s.push_back({ch + "param_embed.weight", {D2, 9}}); s.push_back({ch + "param_embed.bias", {D2}});
    s.push_back({ch + "adapt_norm_gen.1.weight", {3 * D2, D2}}); s.push_back({ch + "adapt_norm_gen.1.bias", {3 * D2}});
    s.push_back({ch + "param_predictor.fc1.weight", {D2 / 2, D2}}); s.push_back({ch + "param_predictor.fc1.bias", {D2 / 2}});
    s.push_back({ch + "param_predictor.fc2.weight", {9, D2 / 2}}); s.push_back({ch + "param_predictor.fc2.bias", {9}});
  }
  auto dpt = [&](const std::string& p, int F, int od, bool gs) {
    const int32_t* oc = c.dpt_out_channels;
    s.push_back({p + "norm.weight", {D2}}); s.push_back({p + "norm.bias", {D2}});
    for (int i = 0; i < 4; ++i) {
      s.push_back({p + "projects." + std::to_string(i) + ".weight", {oc[i], D2, 1, 1}});
      s.push_back({p + "projects." + std::to_string(i) + ".bias", {oc[i]}});
    }
    s.push_back({p + "resize_layers.0.weight", {oc[0], oc[0], 4, 4}}); s.push_back({p + "resize_layers.0.bias", {oc[0]}});
    s.push_back({p + "resize_layers.1.weight", {oc[1], oc[1], 2, 2}}); s.push_back({p + "resize_layers.1.bias", {oc[1]}});
    s.push_back({p + "resize_layers.3.weight", {oc[3], oc[3], 3, 3}}); s.push_back({p + "resize_layers.3.bias", {oc[3]}});
    for (int i = 0; i < 4; ++i) s.push_back({p + "scratch.layer" + std::to_string(i + 1) + "_rn.weight", {F, oc[i], 3, 3}});
    for (int r = 1; r <= 4; ++r) {
      const std::string q = p + "scratch.refinenet" + std::to_string(r) + ".";
      s.push_back({q + "out_conv.weight", {F, F, 1, 1}}); s.push_back({q + "out_conv.bias", {F}});
      for (int u = (r == 4 ? 2 : 1); u <= 2; ++u)
        for (int cv = 1; cv <= 2; ++cv) {
          const std::string nm = q + "resConfUnit" + std::to_string(u) + ".conv" + std::to_string(cv);
          s.push_back({nm + ".weight", {F, F, 3, 3}}); s.push_back({nm + ".bias", {F}});
        }
    }
    s.push_back({p + "scratch.output_conv1.weight", {F / 2, F, 3, 3}}); s.push_back({p + "scratch.output_conv1.bias", {F / 2}});
    s.push_back({p + "scratch.output_conv2.0.weight", {32, F / 2, 3, 3}}); s.push_back({p + "scratch.output_conv2.0.bias", {32}});
    s.push_back({p + "scratch.output_conv2.2.weight", {od, 32, 1, 1}}); s.push_back({p + "scratch.output_conv2.2.bias", {od}});
    if (gs) { s.push_back({p + "input_merger.0.weight", {F / 2, 3, 7, 7}}); s.push_back({p + "input_merger.0.bias", {F / 2}}); }
  };
  if (c.enable_pts) dpt("pts_head.", c.dpt_features, 4, false);
  if (c.enable_depth) dpt("depth_head.", c.dpt_features, 2, false);
  if (c.enable_norm) dpt("norm_head.", c.dpt_features, 4, false);
  if (c.enable_gs) {
    dpt("gs_head.", c.gs_dim, 2, true);
    s.push_back({"gs_renderer.gs_head.0.weight", {c.gs_dim, c.gs_dim / 2, 3, 3}});
    s.push_back({"gs_renderer.gs_head.2.weight", {12, c.gs_dim, 1, 1}});
    s.push_back({"gs_renderer.gs_head.2.bias", {12}});
  }
  return s;
}

}  // namespace

uint16_t h_to16(float f, int dt) { return dt == WM_DT_BF16 ? h_f2bf(f) : h_f2h(f); }

// ------------------------------------------------------------------ small accessors
// (plan() and bind_model() only: the forward reads the bound model)
const Weight* W(const wm_handle* h, const std::string& n) {
  auto it = h->w.find(n);
  return it == h->w.end() ? nullptr : &it->second;
}

}  // namespace wm_host
using namespace wm_host;

extern "C" void wm_host_to_16(const float* in, uint16_t* out, size_t n, int dtype) {
  for (size_t i = 0; i < n; ++i) out[i] = h_to16(in[i], dtype);
}

// ====================================================================================== lifecycle
extern "C" wm_status wm_create(const wm_config* cfg, int device, wm_handle** out) {
  if (!cfg || !out) return WM_ERR_INVALID;
  wm_handle* h = new wm_handle();
  h->cfg = *cfg;
  h->device = device;
  *out = h;
  if (cfg->embed_dim / cfg->num_heads != 64 || cfg->embed_dim / cfg->dino_heads != 64)
    return fail(h, WM_ERR_INVALID, "backbone head_dim must be 64 (reference: 1024/16)");
  if (cfg->embed_dim % 64) return fail(h, WM_ERR_INVALID, "embed_dim must be a multiple of 64");
  if (hipSetDevice(device) != hipSuccess) return fail(h, WM_ERR_HIP, "hipSetDevice failed");
  return WM_OK;
}

extern "C" void wm_destroy(wm_handle* h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  for (auto& hd : h->tconv) for (TconvPack& t : hd) free_tconv(t);
  for (Up1Comp& u : h->up1comp) free_up1comp(u);
  free_tapfold(h->tapfold);
  if (h->hfront) (void)hipEventDestroy(h->hfront);
  for (auto& kv : h->w) {
    if (!kv.second.owned) continue;
    if (kv.second.f32) (void)hipFree(kv.second.f32);
    if (kv.second.w16) (void)hipFree(kv.second.w16);
  }
  if (h->arena && h->arena_owned) (void)hipFree(h->arena);
  for (int i = 0; i < 4; ++i) {
    if (h->hstream[i]) (void)hipStreamDestroy(h->hstream[i]);
    if (h->hjoin[i]) (void)hipEventDestroy(h->hjoin[i]);
  }
  if (h->att_stat_host) (void)hipHostFree(h->att_stat_host);
  if (h->hfork) (void)hipEventDestroy(h->hfork);
  if (h->camstream) (void)hipStreamDestroy(h->camstream);
  if (h->camjoin) (void)hipEventDestroy(h->camjoin);
  if (h->cstream) (void)hipStreamDestroy(h->cstream);
  if (h->cfork) (void)hipEventDestroy(h->cfork);
  if (h->cjoin) (void)hipEventDestroy(h->cjoin);
  for (int k = 0; k < wm_handle::NKIND; ++k)
    for (auto& e : h->ev[k]) { (void)hipEventDestroy(e.a); (void)hipEventDestroy(e.b); }
  if (h->comm.kind == 1 && h->comm.nccl) ncclCommDestroy(h->comm.nccl);
  delete h;
}

extern "C" const char* wm_last_error(const wm_handle* h) { return h ? h->err.c_str() : "null handle"; }

extern "C" wm_status wm_set_weight(wm_handle* h, const char* name, const float* host, const int64_t* shape, int ndim) {
  if (!h || !name || !host || !shape) return WM_ERR_INVALID;
  HIPCHK(h, hipSetDevice(h->device));
  const std::string n(name);
  // strict=False: names outside the spec are ignored
  auto& spec = h->spec;
  if (spec.empty())
    for (auto& kv : param_spec(h->cfg)) spec[kv.first] = kv.second;
  auto it = spec.find(n);
  if (it == spec.end()) return WM_OK;
  std::vector<int64_t> sh(shape, shape + ndim);
  if (sh != it->second) return fail(h, WM_ERR_INVALID, "shape mismatch for " + n);
  size_t numel = 1;
  for (auto s : sh) numel *= (size_t)s;
  Weight& w = h->w[n];
  h->plan_n = -1;  // weight-derived workspace tables (resampled pos_embed, camera init token) are rebuilt by the next wm_reserve
  h->tconv_valid = false;
  if (w.owned) {
    if (w.f32) (void)hipFree(w.f32);
    if (w.w16) (void)hipFree(w.w16);
  }
  w.f32 = nullptr; w.w16 = nullptr; w.owned = true; w.tap_major = false;
  w.shape = sh;
  w.set = true;
  const WKind k = classify(n, ndim);
  if (k == WK_F32) {
    HIPCHK(h, hipMalloc((void**)&w.f32, std::max<size_t>(numel, 4) * 4));
    HIPCHK(h, hipMemcpy(w.f32, host, numel * 4, hipMemcpyHostToDevice));
    if (ends_with(n, "pos_embed") || ends_with(n, "init_token")) w.host.assign(host, host + numel);
    if (n.find(".resize_layers.0.bias") != std::string::npos || n.find(".resize_layers.1.bias") != std::string::npos ||
        ends_with(n, ".scratch.refinenet1.out_conv.bias") || is_tapfold_source(n))
      w.host.assign(host, host + numel);
    return WM_OK;
  }
  // the ConvTranspose / layer_rn pairs that wm_reserve composes into one token-resolution GEMM (build_tconv) are kept in fp32 on the host
  if (n.find(".resize_layers.0.weight") != std::string::npos || n.find(".resize_layers.1.weight") != std::string::npos ||
      ends_with(n, ".scratch.layer1_rn.weight") || ends_with(n, ".scratch.layer2_rn.weight") ||
      ends_with(n, ".scratch.refinenet1.out_conv.weight") || ends_with(n, ".scratch.output_conv1.weight") ||   // (+ build_up1comp)
      is_tapfold_source(n))                                                                                    // (+ build_tapfold)
    w.host.assign(host, host + numel);
  const int dt = k == WK_LIN16_BACKBONE ? h->cfg.backbone_dtype : h->cfg.head_dtype;
  std::vector<uint16_t> r;
  if (k == WK_LIN16_BACKBONE || k == WK_LIN16_HEAD) {
    const int N = (int)sh[0];
    const int K = (int)(numel / N);
    const int Kp = ru(K, 64);
    r.assign((size_t)N * Kp, 0);
    for (int i = 0; i < N; ++i)
      for (int j = 0; j < K; ++j) r[(size_t)i * Kp + j] = h_to16(host[(size_t)i * K + j], dt);
    w.k16 = Kp;
  } else if (k == WK_CONV16_HEAD) {  // [Cout][Cin][kh][kw] -> [Cout][kh][kw][Cin]
    const int Co = (int)sh[0], Ci = (int)sh[1], kh = (int)sh[2], kw = (int)sh[3];
    r.resize(numel);
    for (int o = 0; o < Co; ++o)
      for (int c = 0; c < Ci; ++c)
        for (int y = 0; y < kh; ++y)
          for (int x = 0; x < kw; ++x)
            r[(((size_t)o * kh + y) * kw + x) * Ci + c] = h_to16(host[(((size_t)o * Ci + c) * kh + y) * kw + x], dt);
    w.k16 = kh * kw * Ci;
    if (kh == 3 && kw == 3 && ends_with(n, "output_conv1.weight")) {
      // a second, tap-major copy [tap][Cout][Cin] behind the first: the B operand of the low-resolution tap GEMM (upconv.hip)
      r.resize(2 * numel);
      for (int o = 0; o < Co; ++o)
        for (int t = 0; t < 9; ++t)
          for (int c = 0; c < Ci; ++c) r[numel + ((size_t)t * Co + o) * Ci + c] = r[((size_t)o * 9 + t) * Ci + c];
      w.tap_major = true;
    }
  } else {  // ConvTranspose2d [Cin][Cout][k][k] -> rows (i*k + j)*Cout + co, K = Cin
    const int Ci = (int)sh[0], Co = (int)sh[1], kk = (int)sh[2];
    r.resize(numel);
    for (int c = 0; c < Ci; ++c)
      for (int o = 0; o < Co; ++o)
        for (int i = 0; i < kk; ++i)
          for (int j = 0; j < kk; ++j)
            r[((size_t)(i * kk + j) * Co + o) * Ci + c] = h_to16(host[(((size_t)c * Co + o) * kk + i) * kk + j], dt);
    w.k16 = Ci;
  }
  HIPCHK(h, hipMalloc(&w.w16, r.size() * 2));
  HIPCHK(h, hipMemcpy(w.w16, r.data(), r.size() * 2, hipMemcpyHostToDevice));
  return WM_OK;
}

// The value a parameter has in a freshly constructed reference model, where that value is deterministic: what a tensor
// missing from the checkpoint keeps under load_state_dict(strict=False) (huggingface_hub mixin, worldmirror.py:13,16).
// LayerNorm weight 1 / bias 0 (torch default); LayerScale gamma = init_values: 1.0 in the DINOv2 encoder
// (visual_transformer.py:152-160), 0.01 in the multi-view blocks and the camera trunk (visual_transformer.py:65,
// camera_head.py:24).  Everything else (Linear / conv weights and biases, learned tokens) is RANDOM in the reference
// (trunc_normal / kaiming-uniform / normal(1e-6)): not reproducible, filled with 0 and reported through wm_missing_name.
static float init_value_of(const std::string& n) {
  const bool norm = n.find(".norm1.") != std::string::npos || n.find(".norm2.") != std::string::npos || n.find(".norm.") != std::string::npos ||
                    n.find("q_norm.") != std::string::npos || n.find("k_norm.") != std::string::npos || n.find("token_norm.") != std::string::npos ||
                    n.find("out_norm.") != std::string::npos;
  if (norm) return ends_with(n, ".weight") ? 1.0f : 0.0f;
  if (ends_with(n, ".gamma")) return n.find(".patch_embed.") != std::string::npos ? 1.0f : 0.01f;
  return 0.0f;
}

extern "C" wm_status wm_finalize_weights(wm_handle* h, int* missing) {
  if (!h) return WM_ERR_INVALID;
  HIPCHK(h, hipSetDevice(h->device));
  h->missing.clear();
  for (auto& kv : param_spec(h->cfg)) {
    auto it = h->w.find(kv.first);
    if (it != h->w.end() && it->second.set) continue;
    h->missing.push_back(kv.first);  // strict=False: a missing tensor keeps its init value (see init_value_of)
    size_t numel = 1;
    for (auto s : kv.second) numel *= (size_t)s;
    std::vector<float> z(numel, init_value_of(kv.first));
    wm_status st = wm_set_weight(h, kv.first.c_str(), z.data(), kv.second.data(), (int)kv.second.size());
    if (st != WM_OK) return st;
    h->w[kv.first].set = false;
  }
  if (missing) *missing = (int)h->missing.size();
  h->finalized = true;
  return WM_OK;
}

extern "C" wm_status wm_share_weights(wm_handle* dst, const wm_handle* src) {
  if (!dst || !src || dst == src) return WM_ERR_INVALID;
  if (!src->finalized) return fail(dst, WM_ERR_STATE, "source weights not finalized");
  if (memcmp(&dst->cfg, &src->cfg, sizeof(wm_config)) != 0 || dst->device != src->device)
    return fail(dst, WM_ERR_INVALID, "wm_share_weights: configuration or device differs");
  for (auto& kv : dst->w) {
    if (!kv.second.owned) continue;
    if (kv.second.f32) (void)hipFree(kv.second.f32);
    if (kv.second.w16) (void)hipFree(kv.second.w16);
  }
  dst->w = src->w;
  for (auto& kv : dst->w) kv.second.owned = false;
  dst->spec = src->spec;
  dst->missing = src->missing;
  dst->finalized = true;
  dst->plan_n = -1;
  dst->tconv_valid = false;
  return WM_OK;
}

extern "C" const char* wm_missing_name(const wm_handle* h, int i) {
  return (h && i >= 0 && (size_t)i < h->missing.size()) ? h->missing[i].c_str() : nullptr;
}
