// Host orchestrator + C ABI (include/wm_hip.h) of the MI355X-native WorldMirror forward pass.
//
// One wm_handle = one process/GPU: owns the repacked weights and a workspace arena, and turns
// WorldMirror.forward (reference src/models/models/worldmirror.py:120-216) into a fixed sequence of
// HIP kernel launches on the caller's stream.  No torch, no hidden per-call allocation once the
// workspace for a shape exists.  The other entries of the C ABI are in wm_api_ops.cpp (wm_op_*) and
// wm_api_scene.cpp (ingest, masks, rasteriser, densify, MCMC, losses, bilagrid, appearance).
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>
#include <pthread.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/wm_hip.h"
#include "wm_kernels.h"

namespace {

inline int ru(int x, int m) { return (x + m - 1) / m * m; }

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
inline uint16_t h_to16(float f, int dt) { return dt == WM_DT_BF16 ? h_f2bf(f) : h_f2h(f); }

struct Weight {
  std::vector<int64_t> shape;
  float* f32 = nullptr;  // device
  void* w16 = nullptr;   // device 16-bit repack
  int k16 = 0;           // padded K of the repack
  bool tap_major = false;  // w16 holds a second copy [tap][Cout][Cin] of a 3x3 conv weight behind the first (numel elements in)
  std::vector<float> host;  // kept only for the few tensors the host needs (pos_embed, init_token)
  bool set = false;
  bool owned = true;  // false: device memory belongs to another handle (wm_share_weights)
};

// the composed ConvTranspose -> 3x3 conv of a DPT head level (build_tconv below)
struct TconvPack {
  void* w16 = nullptr;        // [k^2 * 256][4 * Cin] 16-bit: row (phase, co), the phase's neighbour matrices side by side
  float* bias_rep = nullptr;  // [k^2][256]: (sum_tap W_rn[tap]) b_ct, once per phase
  float* bmiss = nullptr;     // [9][256]: W_rn[tap] b_ct (wm_launch_tconv_border)
  unsigned list[16] = {0};
  int k = 0, cin = 0;
};
static void free_tconv(TconvPack& t) {
  if (t.w16) (void)hipFree(t.w16);
  if (t.bias_rep) (void)hipFree(t.bias_rep);
  if (t.bmiss) (void)hipFree(t.bmiss);
  t = TconvPack();
}

static hipError_t build_tconv(int dt, int k, int Cin, int Cm, int F_, const float* wct, const float* bct, const float* wrn, TconvPack& out, hipStream_t s);
// refinenet1.out_conv (1x1) composed into the nine tap matrices of output_conv1 (upconv.hip): the tap GEMM then reads the last fusion block's
// 16-bit tensor directly — W[tap][co][ci] = sum_c W_oc1[co][c][tap] W_out[c][ci], bias[tap][co] = sum_c W_oc1[co][c][tap] b_out[c] (build_up1comp)
struct Up1Comp {
  void* w16 = nullptr;     // [9 Co][F] 16-bit
  float* bias = nullptr;   // [9 Co]
  int co = 0;
};
static void free_up1comp(Up1Comp& u) {
  if (u.w16) (void)hipFree(u.w16);
  if (u.bias) (void)hipFree(u.bias);
  u = Up1Comp();
}
static hipError_t build_up1comp(int dt, int F_, int Co, const float* woc1, const float* wout, const float* bout, Up1Comp& out, hipStream_t s);

// The DPT heads' tap front shared between heads (tuning tap_shared): LayerNorm(2D) -> projects.i (dense_head.py:53,204-208) with each head's
// LayerNorm affine folded into its projection, W'_h = W_h diag(gamma_h), b'_h = b_h + W_h beta_h, the heads' rows one under the other: all heads
// then read the SAME normalised tap and one GEMM per tap serves them all (build_tapfold below)
struct TapFold {
  void* w16[4] = {nullptr, nullptr, nullptr, nullptr};      // per tap [nh * oc_i][Kp] 16-bit
  float* bias[4] = {nullptr, nullptr, nullptr, nullptr};    // per tap [nh * oc_i]
  int heads[4] = {0, 0, 0, 0}, nh = 0;                      // the group's heads (HeadId), in the order of their row blocks
  bool valid = false;                                       // false: no group, or a folded weight left the operand type's range (direct form)
};
static void free_tapfold(TapFold& t) {
  for (int i = 0; i < 4; ++i) {
    if (t.w16[i]) (void)hipFree(t.w16[i]);
    if (t.bias[i]) (void)hipFree(t.bias[i]);
  }
  t = TapFold();
}
// one tap: W[h] [oc][K], b[h] [oc], gamma[h], beta[h] [K] (host fp32) -> w16 [nh oc][Kp], bias [nh oc] on the device; *in_range = false (and nothing
// allocated) when a folded weight or bias is not finite, or a weight exceeds the f16 maximum for f16 operands
static hipError_t build_tapfold(int dt, int nh, int oc, int K, int Kp, const float* const* Wh, const float* const* bh, const float* const* gamma,
                                const float* const* beta, void** w16_out, float** bias_out, bool* in_range);

// ------------------------------------------------------------------ bound model
// Everything the forward reads, as device pointers and the few ints taken from shapes: filled by bind_model() at the end of plan(), the one
// point where both the weights and the shape are final (wm_set_weight / wm_share_weights / wm_set_workspace invalidate the plan).  The
// forward addresses nothing by name.  A null pointer below is an operand the layer does not have, and is marked so.
enum HeadId { HD_DEPTH = 0, HD_PTS, HD_NORM, HD_GS, HD_COUNT };   // the DPT heads in the order the forward runs them
const char* const kHeadPrefix[HD_COUNT] = {"depth_head.", "pts_head.", "norm_head.", "gs_head."};
inline bool head_enabled(const wm_config& c, int id) {
  return id == HD_DEPTH ? c.enable_depth : id == HD_PTS ? c.enable_pts : id == HD_NORM ? c.enable_norm : c.enable_gs;
}
struct Lin16 { const void* w = nullptr; const float* b = nullptr; };                   // 16-bit matrix [N][Kpad] + fp32 bias
struct Lin32 { const float* w = nullptr; const float* b = nullptr; int N = 0, K = 0; };   // fp32 Linear [N][K] + bias
struct Norm { const float* w = nullptr; const float* b = nullptr; };
struct ConvW { const void* w16 = nullptr; const float* bias = nullptr; int cin = 0, cout = 0; };   // bias null: the conv has none
struct BlockW {            // one transformer block of the backbone (16-bit operands)
  Norm norm1, norm2;
  Lin16 qkv, proj, fc1, fc2;
  Norm q_norm, k_norm;     // null in the DINO blocks (no q/k-norm)
  const float *ls1 = nullptr, *ls2 = nullptr;
};
struct CamBlockW {         // one block of the camera head's trunk (fp32)
  Norm norm1, norm2;
  Lin32 qkv, proj, fc1, fc2;
  const float *ls1 = nullptr, *ls2 = nullptr;
};
struct HeadW {             // one DPT head
  Norm norm;
  Lin16 proj[4];
  Lin16 resize[2];         // ConvTranspose2d (kernel = stride) as a GEMM
  ConvW resize3;
  ConvW rn[4];             // layer{i+1}_rn (no bias)
  ConvW rcu[4][2][2];      // [refinenet - 1][resConfUnit - 1][conv - 1]; refinenet4 has no unit 1
  ConvW out_conv[4];       // Cin = Cout = the head's feature width (checked by bind_model)
  ConvW oc1;               // output_conv1
  const void* oc1_tap = nullptr;      // its tap-major copy [tap][Cout][Cin], null when the repack made none
  const Up1Comp* comp = nullptr;      // refinenet1.out_conv composed into it, null when wm_reserve built none for this Cout
  ConvW oc2_0;             // output_conv2.0
  Lin32 oc2_2;             // output_conv2.2 (1x1, fp32)
  Lin16 merger;            // input_merger.0 (Gaussian head only)
  ConvW gs0, gs2;          // gs_renderer.gs_head.0 (no bias) / .2 (Gaussian head only)
  const TconvPack* tconv[2] = {nullptr, nullptr};   // null: no composed form for this level
};
struct Model {
  Lin16 patch_proj;
  const float *cls_token = nullptr, *register_tokens = nullptr, *cam_token = nullptr, *reg_token = nullptr;
  Norm dino_norm;
  std::vector<BlockW> dino, frame, global;
  Lin32 pose_embed[2], ray_embed[2];   // enable_cond only
  Lin16 depth_fc1, depth_fc2;
  Norm cam_token_norm, cam_out_norm;
  Lin32 cam_param_embed, cam_adapt, cam_pred_fc1, cam_pred_fc2;
  std::vector<CamBlockW> cam;
  HeadW head[HD_COUNT];
};
struct HeadBufs {          // the workspace of one head SLOT (the k-th head a call runs, whichever head that is)
  void *T16 = nullptr, *P16 = nullptr, *P16b = nullptr;   // P16b only with two or more slots
  float *f0 = nullptr, *f1 = nullptr, *f2 = nullptr, *f3in = nullptr, *f3 = nullptr;
  float* rn[4] = {nullptr, nullptr, nullptr, nullptr};
  float* s[4] = {nullptr, nullptr, nullptr, nullptr};
};
struct Workspace {
  float *Xd = nullptr, *Xv = nullptr;
  uint16_t* A16 = nullptr;
  char* QKV16 = nullptr;
  void *O16 = nullptr, *H16 = nullptr;
  float* tap[4] = {nullptr, nullptr, nullptr, nullptr};
  char* KVG = nullptr;
  float *ATT_PO = nullptr, *ATT_ML = nullptr, *LN_STATS = nullptr;
  int *ATT_FLAGS = nullptr, *ATT_HINT = nullptr, *ATT_STAT = nullptr, *LN_SYNC = nullptr;
  uint16_t* ZERO256 = nullptr;
  float *rope_cos = nullptr, *rope_sin = nullptr, *dino_pos = nullptr;
  float *pr_in = nullptr, *pr_h = nullptr, *pose_tok = nullptr, *ray_tok = nullptr;
  float *cam_tok_local = nullptr, *cam_tok = nullptr, *cam_e = nullptr, *cam_mod = nullptr, *cam_h = nullptr, *cam_a = nullptr, *cam_qkv = nullptr;
  float *cam_o = nullptr, *cam_f = nullptr, *cam_pred = nullptr, *cam_delta = nullptr, *cam_init = nullptr, *cam_params = nullptr;
  HeadBufs hb[4];
  void* gs_im2col = nullptr;            // enable_gs only
  float* dpt_pos[4] = {nullptr, nullptr, nullptr, nullptr};
  float *posx[2] = {nullptr, nullptr}, *posy[2] = {nullptr, nullptr};   // [0] the dense heads' width, [1] the Gaussian head's
};

struct EvPair { hipEvent_t a, b; };

struct Comm {
  int kind = 0;  // 0 none, 1 rccl, 2 local
  int rank = 0, world = 1;
  ncclComm_t nccl = nullptr;
  wm_local_group* grp = nullptr;
};

}  // namespace

struct wm_local_group {
  int world;
  pthread_barrier_t bar;
  std::vector<void*> recv;
};

struct wm_handle {
  wm_config cfg;
  int device = 0;
  std::string err;
  std::unordered_map<std::string, Weight> w;
  std::map<std::string, std::vector<int64_t>> spec;
  bool finalized = false;
  Comm comm;
  // workspace
  char* arena = nullptr;
  size_t arena_bytes = 0;
  bool arena_owned = true;   // false: caller-provided (wm_set_workspace)
  int plan_n = -1, plan_nt = -1, plan_H = -1, plan_W = -1;
  TconvPack tconv[HD_COUNT][2];             // per head and level: rebuilt by wm_reserve after a weight change
  bool tconv_valid = false;
  Up1Comp up1comp[HD_COUNT];                // per head, rebuilt with the token-conv packs
  TapFold tapfold;                          // the heads' shared tap front, rebuilt with them
  std::vector<std::string> missing;  // names wm_finalize_weights filled with their init values
  // the weights and the workspace (with its shape-dependent device tables) as the forward reads them: bound by plan()
  Model m;
  Workspace ws;
  // the DPT heads are mutually independent: each runs on its own stream (forked/joined with events)
  hipStream_t hstream[4] = {nullptr, nullptr, nullptr, nullptr};
  hipEvent_t hfork = nullptr, hjoin[4] = {nullptr, nullptr, nullptr, nullptr};
  hipEvent_t hfront = nullptr;   // behind the heads' shared tap front on the caller's stream: the forked heads start from it
  // K/V all-gather of the sharded forward runs on its own queue, under the attention over the local keys
  hipStream_t cstream = nullptr;
  hipEvent_t cfork = nullptr, cjoin = nullptr;
  // the camera head (HBM-bound weight streaming) runs beside the DPT heads (MFMA-bound) on its own queue
  hipStream_t camstream = nullptr;
  hipEvent_t camjoin = nullptr;
  // fast-attention fallback statistics per call site (WmAttnArgs::unit_stat): pinned host copy written by an async D2H at the end of
  // every forward, the last value seen per site, and the calls left in general-kernel-only mode
  int* att_stat_host = nullptr;
  int att_stat_n = 0;
  std::vector<int> att_seen, att_general_ttl;
  // profiling
  bool prof = false;
  static constexpr int NKIND = 13;
  std::vector<EvPair> ev[NKIND];
  size_t ev_used[NKIND] = {};
};

namespace {

wm_status fail(wm_handle* h, wm_status st, const std::string& msg) {
  if (h) h->err = msg;
  return st;
}
#define HIPCHK(h, e)                                                                                   \
  do {                                                                                                 \
    hipError_t _e = (e);                                                                               \
    if (_e != hipSuccess)                                                                              \
      return fail(h, WM_ERR_HIP, std::string(hipGetErrorString(_e)) + " at " + __FILE__ + ":" + std::to_string(__LINE__)); \
  } while (0)

bool ends_with(const std::string& s, const char* suf) {
  const size_t n = strlen(suf);
  return s.size() >= n && s.compare(s.size() - n, n, suf) == 0;
}
bool starts_with(const std::string& s, const char* p) { return s.compare(0, strlen(p), p) == 0; }
// the tensors build_tapfold composes (kept in fp32 on the host): a DPT head's norm.{weight,bias} and projects.i.{weight,bias}
bool is_tapfold_source(const std::string& n) {
  for (const char* p : {"pts_head.", "depth_head.", "norm_head.", "gs_head."})
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
  const bool head = starts_with(n, "pts_head.") || starts_with(n, "depth_head.") || starts_with(n, "norm_head.") || starts_with(n, "gs_head.");
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

// ------------------------------------------------------------------ small accessors
// (plan() and bind_model() only: the forward reads the bound model)
const Weight* W(const wm_handle* h, const std::string& n) {
  auto it = h->w.find(n);
  return it == h->w.end() ? nullptr : &it->second;
}

struct Dims {
  int n, nt, H, W, gh, gw, hw, Td, P, psi, D, heads, R, Md, Mv, Mx, kpad_patch, kpad_depth, world, chunk;
  int gh2, gw2;
};

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

#define WM_TUNE_UNSET(name_, key_) -1,
#define WM_TUNE_NAME(name_, key_) key_,
int wm_tuning[WM_TUNE_COUNT] = {WM_TUNE_KEYS(WM_TUNE_UNSET)};
static const char* const wm_tuning_keys[WM_TUNE_COUNT] = {WM_TUNE_KEYS(WM_TUNE_NAME)};

extern "C" int wm_set_tuning(const char* key, int value) {
  for (int i = 0; i < WM_TUNE_COUNT; ++i)
    if (key && strcmp(key, wm_tuning_keys[i]) == 0) { wm_tuning[i] = value; return 0; }
  return -1;
}

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

// ====================================================================================== workspace
extern "C" size_t wm_workspace_bytes(const wm_handle* h, int n_local, int n_total, int H, int W) {
  if (!h) return 0;
  const Dims d = make_dims(h, n_local, n_total, H, W);
  size_t tot = 0;
  for (auto& kv : arena_layout(h, d)) tot += kv.second;
  return tot;
}

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

// Builds the workspace for a shape: arena (library-owned unless the caller gave one), the composed head weights, the bound model
// (bind_model) and the shape- / weight-derived device tables.  Called by wm_reserve only — never from the forward pass.
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
  h->plan_n = d.n; h->plan_nt = d.nt; h->plan_H = d.H; h->plan_W = d.W;
  return WM_OK;
}

// ---------------------------------------------------------------- profiling helpers
struct ProfScope {
  wm_handle* h; int kind; hipStream_t s; EvPair* e = nullptr;
  ProfScope(wm_handle* h_, int k, hipStream_t s_) : h(h_), kind(k), s(s_) {
    if (!h->prof) return;
    auto& v = h->ev[kind];
    if (h->ev_used[kind] == v.size()) {
      EvPair p;
      (void)hipEventCreate(&p.a); (void)hipEventCreate(&p.b);
      v.push_back(p);
    }
    e = &v[h->ev_used[kind]++];
    (void)hipEventRecord(e->a, s);
  }
  ~ProfScope() { if (e) (void)hipEventRecord(e->b, s); }
};

// ---------------------------------------------------------------- collective
wm_status comm_allgather(wm_handle* h, const void* send, void* recv, size_t bytes, hipStream_t s) {
  ProfScope ps(h, 12, s);   // timing kind 12: the collective, on the queue it runs on (the compute queue unless tuning comm_overlap = 1)
  Comm& cm = h->comm;
  if (cm.kind == 1) {
    if (wm_tune(WM_TUNE_COMM_P2P, 0) == 1) {
      // Direct all-gather (opt-in, tuning comm_p2p = 1 / bench.py --gather p2p): every rank sends its chunk to every peer and
      // receives every peer's chunk as ONE group of point-to-point operations, so each of the 7 xGMI links of a GPU carries one
      // chunk in each direction at once (~0.29 ms per layer link-bound at C4, against ~2.1 ms if the all-gather
      // runs as a ring).  Not the default: no multi-GPU node was available to any build round, and RCCL may already pick a
      // direct algorithm for ncclAllGather on a fully connected node — the first 8-GPU run has to say.
      if (ncclGroupStart() != ncclSuccess) return fail(h, WM_ERR_COMM, "ncclGroupStart failed");
      for (int r = 0; r < cm.world; ++r) {
        if (r == cm.rank) continue;
        if (ncclSend(send, bytes, ncclInt8, r, cm.nccl, s) != ncclSuccess) return fail(h, WM_ERR_COMM, "ncclSend failed");
        if (ncclRecv((char*)recv + (size_t)r * bytes, bytes, ncclInt8, r, cm.nccl, s) != ncclSuccess) return fail(h, WM_ERR_COMM, "ncclRecv failed");
      }
      if (ncclGroupEnd() != ncclSuccess) return fail(h, WM_ERR_COMM, "ncclGroupEnd failed");
      HIPCHK(h, hipMemcpyAsync((char*)recv + (size_t)cm.rank * bytes, send, bytes, hipMemcpyDeviceToDevice, s));
      return WM_OK;
    }
    if (ncclAllGather(send, recv, bytes, ncclInt8, cm.nccl, s) != ncclSuccess) return fail(h, WM_ERR_COMM, "ncclAllGather failed");
    return WM_OK;
  }
  if (cm.kind == 2) {
    wm_local_group* g = cm.grp;
    g->recv[cm.rank] = recv;
    HIPCHK(h, hipStreamSynchronize(s));
    pthread_barrier_wait(&g->bar);
    for (int r = 0; r < g->world; ++r)
      HIPCHK(h, hipMemcpyAsync((char*)g->recv[r] + (size_t)cm.rank * bytes, send, bytes, hipMemcpyDeviceToDevice, s));
    HIPCHK(h, hipStreamSynchronize(s));
    pthread_barrier_wait(&g->bar);
    return WM_OK;
  }
  return fail(h, WM_ERR_COMM, "sharded forward without a communicator");
}

// ---------------------------------------------------------------- building blocks
struct Ctx {
  wm_handle* h; Dims d; hipStream_t s; int bdt, hdt;
  int attn_site = 0;   // attention call sites passed so far in this forward (index of the site's sticky fallback hints, ATT_HINT)
};

#define LCHK(c, e)                                                                                            \
  do {                                                                                                        \
    hipError_t _e = (e);                                                                                      \
    if (_e != hipSuccess)                                                                                     \
      return fail((c).h, WM_ERR_HIP, std::string(hipGetErrorString(_e)) + " at " + __FILE__ + ":" + std::to_string(__LINE__)); \
  } while (0)

wm_status gemm(Ctx& c, int dt, int epi, const void* A, int lda, const void* Wp, int ldw, void* C, int ldc, const float* bias,
               const float* gamma, int M, int N, int K, WmGemmArgs* extra = nullptr, int prof_kind = -1, bool* ln_fused = nullptr) {
  WmGemmArgs a;
  if (extra) a = *extra; else memset(&a, 0, sizeof(a));
  a.A = A; a.W = Wp; a.C = C; a.bias = bias; a.gamma = gamma;
  a.M = M; a.N = N; a.K = K; a.lda = lda; a.ldw = ldw; a.ldc = ldc; a.dtype = dt; a.epi = epi;
  // timing kinds by kernel instantiation: the three epilogues that carry the transformer blocks, the rest under 2
  ProfScope ps(c.h, prof_kind >= 0 ? prof_kind : epi == WM_EPI_QKV ? 5 : epi == WM_EPI_RESID ? 6 : epi == WM_EPI_GELU_T16 ? 7 : 2, c.s);
  const bool fuse = a.ln_out != nullptr && wm_gemm_fuses_ln(a);
  if (!fuse) a.ln_out = nullptr;
  if (ln_fused) *ln_fused = fuse;
  LCHK(c, wm_launch_gemm(a, c.s));
  if (fuse) LCHK(c, wm_launch_gemm_ln_fallback(a, c.s));   // bands whose rendezvous timed out (normally none: every block exits at entry)
  return WM_OK;
}

// a: the caller sets, by field name, what differs from zero
wm_status layernorm(Ctx& c, const WmLnArgs& a) {
  LCHK(c, wm_launch_layernorm(a, c.s));
  return WM_OK;
}

// Block.forward (block.py:72-93) on the fp32 residual stream X [M][D]; seq_len = attention span.
// tap_half: when non-null, the block's output (the value its last GEMM stores to X) is also written to tap_half[row * 2D + col]
// by that GEMM's epilogue — the cat([frame_out, global_out], -1) of visual_transformer.py:337-339 without a copy pass.
// next_norm1: norm1 of the block that follows on the same stream X (null = none): it is then computed by this block's fc2
// epilogue when the shape allows (wm_gemm_fuses_ln) and *ln1_ready tells the caller to pass ln1_done to that block.
wm_status backbone_block(Ctx& c, const BlockW& w, float* X, int M, int seq_len, int heads, float eps,
                         bool rope, int tokens_per_view, int patch_start, bool is_global, float* tap_half = nullptr,
                         bool ln1_done = false, const Norm* next_norm1 = nullptr, bool* ln1_ready = nullptr) {
  wm_handle* h = c.h;
  const Dims& d = c.d;
  const Workspace& ws = h->ws;
  const int D = d.D, dt = c.bdt;
  uint16_t* A16 = ws.A16;
  char* QKV16 = ws.QKV16;
  const size_t hsz = (size_t)M * D * 2;  // bytes of one of Q/K/V
  void* Q16 = QKV16; void* K16 = QKV16 + hsz; void* V16 = QKV16 + 2 * hsz;
  void* O16 = ws.O16;
  void* H16 = ws.H16;
  wm_status st;
  if (ln1_ready) *ln1_ready = false;
  WmLnArgs ln{};   // norm1 / norm2 of the M rows of X into A16
  ln.x = X; ln.ld_in = D; ln.y = A16; ln.ld_out = D; ln.D = D; ln.eps = eps; ln.groups = 1; ln.rows_per_group = M; ln.dtype = dt;
  if (!ln1_done) {
    ln.w = w.norm1.w; ln.b = w.norm1.b;
    st = layernorm(c, ln);
    if (st) return st;
  }
  // the residual GEMMs carry the LayerNorm that follows them when the launch allows it (gemm.hip epilogue_resid_ln)
  auto fuse_args = [&](WmGemmArgs& ex, const Norm& n) {
    ex.ln_out = A16; ex.ln_ld = D; ex.ln_w = n.w; ex.ln_b = n.b; ex.ln_eps = eps;
    ex.ln_stats = ws.LN_STATS;
    int* sync = ws.LN_SYNC;
    ex.ln_sync = sync; ex.ln_fallback = sync + ((size_t)d.Mx / 16 + 2) * 2;
  };
  {  // QKV projection with q/k-norm + RoPE + head-major relayout fused into the epilogue (attention.py:50-56)
    WmGemmArgs ex;
    memset(&ex, 0, sizeof(ex));
    WmQkvArgs& a = ex.qkv;
    a.q = Q16; a.k = K16; a.v = V16;
    a.qn_w = w.q_norm.w; a.qn_b = w.q_norm.b; a.kn_w = w.k_norm.w; a.kn_b = w.k_norm.b;   // (null in the DINO blocks)
    if (rope) { a.rope_cos = ws.rope_cos; a.rope_sin = ws.rope_sin; }
    a.M = M; a.H = heads; a.head_stride = M; a.tokens_per_view = tokens_per_view; a.patch_start = patch_start; a.grid_w = d.gw;
    a.q_scale = 0.125f * 1.4426950408889634f; a.dtype = dt;  // 1/sqrt(64) * log2(e): the attention kernel works in base 2
    st = gemm(c, dt, WM_EPI_QKV, A16, D, w.qkv.w, D, nullptr, 0, w.qkv.b, nullptr, M, 3 * D, D, &ex);
    if (st) return st;
  }
  {
    WmAttnArgs a;
    memset(&a, 0, sizeof(a));
    a.Q = Q16; a.O = O16; a.H = heads; a.q_rows = M; a.q_head_stride = M; a.dtype = dt;
    const bool force_gather = wm_tune(WM_TUNE_FORCE_GATHER, 0) > 0;  // 1-rank test of the collective path (tests/test_gpu_sharded.py)
    // Opt-in (tuning comm_overlap = 1; default: the gather on the compute queue): the overlapped form is
    // exercised by 8 in-process ranks on one GPU (tests/test_gpu_fullsize.py), but RCCL has not run it on real links yet
    // (no multi-GPU node was available to any round): the simpler event-free path is the default until one 8-GPU run of both,
    // compared bit for bit, is on record.  The second queue is safe here: between fork and join the compute queue runs only
    // the attention kernels, which contain no packed-fp32 instruction (the hazard described at the DPT heads below needs one;
    // tests/test_kernel_resources_cpu.py disassembles them)
    a.part_o = ws.ATT_PO; a.part_ml = ws.ATT_ML; a.max_splits = WM_ATTN_MAX_SPLITS;
    a.unit_flags = ws.ATT_FLAGS;
    const size_t hint_n = wm_attention_max_blocks((int)d.Mx, d.P < d.Td ? d.P : d.Td, d.heads);
    const int site = c.attn_site++;
    int* const hint0 = ws.ATT_HINT + (size_t)site * 3 * hint_n;
    int* const stat0 = ws.ATT_STAT + (size_t)site * 3;
    a.unit_hint = hint0; a.unit_stat = stat0;
    bool general_only = false;
    if (site * 3 < h->att_stat_n) {
      // host policy from the (asynchronously mirrored, possibly one or two forwards old) counter: a quarter of the site's fast-kernel
      // units on the general kernel since the last look -> general kernel only for the next WM_ATTN_HINT_TTL calls
      const int cur = h->att_stat_host[site * 3], delta = cur - h->att_seen[site * 3];
      h->att_seen[site * 3] = cur;
      const long units = (long)((seq_len + 511) / 512) * (M / (seq_len > 0 ? seq_len : 1)) * heads;
      if (delta > 0 && (long)delta * 4 >= units) h->att_general_ttl[site * 3] = WM_ATTN_HINT_TTL;
      if (h->att_general_ttl[site * 3] > 0) { --h->att_general_ttl[site * 3]; general_only = true; }
    }
    const bool sharded = is_global && (d.world > 1 || (force_gather && h->comm.kind != 0));
    const int ntpc = (M + 63) / 64;  // key tiles per rank chunk
    const bool overlap = wm_tune(WM_TUNE_COMM_OVERLAP, 0) != 0;
    // every launch argument set of the overlapped form is checked BEFORE the fork: a rank that returned between the fork and
    // the collective would leave its peers waiting in the all-gather
    bool overlap_ok = sharded && overlap && d.world > 1 && ntpc >= 16;
    if (overlap_ok) {
      WmAttnArgs t = a;
      t.force_partial = 1; t.K = K16; t.V = V16; t.seq_len = M; t.kv_head_stride = M; t.kv_chunks = 1;
      overlap_ok = wm_attention_variant(t) >= 0;
      t.kv_chunks = d.world - 1 > 1 ? d.world - 1 : 2; t.kv_rows_per_chunk = M; t.kv_chunk_stride = (long long)(2 * hsz / 2);
      overlap_ok = overlap_ok && wm_attention_variant(t) >= 0;
    }
    if (overlap_ok) {
      // ---- K/V all-gather UNDER the attention over this rank's own keys: the collective runs on the handle's
      // communication queue as soon as the QKV epilogue has written K|V; the compute queue meanwhile attends the local chunk
      // (1 / world of the keys: about the gather's own duration at 8 ranks), then the remote chunks — the gathered buffer's
      // ranges [0, rank) and (rank, world) — and one combine pass over all partial slots.  Softmax partials make the order
      // of the three key ranges irrelevant (attention.hip attn_combine_kernel).
      if (!h->cstream) {
        LCHK(c, hipStreamCreateWithFlags(&h->cstream, hipStreamNonBlocking));
        LCHK(c, hipEventCreateWithFlags(&h->cfork, hipEventDisableTiming));
        LCHK(c, hipEventCreateWithFlags(&h->cjoin, hipEventDisableTiming));
      }
      char* KVG = ws.KVG;
      const int rank = h->comm.rank, world = d.world;
      LCHK(c, hipEventRecord(h->cfork, c.s));
      // slice counts: minimise rounds x tiles per block over the resident slots, per launch (uniform slices only)
      static const int ncu = [] { hipDeviceProp_t pr; int dv = 0; (void)hipGetDevice(&dv); return hipGetDeviceProperties(&pr, dv) == hipSuccess ? pr.multiProcessorCount : 256; }();
      // Slice count of one piecewise launch over `ntiles` key tiles: the unit size and residency are those of the kernel THAT launch
      // takes (with one view per rank the local launch is a 256-row-unit kernel and the remote ones attn_v4 with 512-row units at
      // one block per CU), so each launch asks wm_attention_geometry with its own arguments
      auto pick = [&](int chunks, int smax) {
        WmAttnArgs g = a;
        g.force_partial = 1; g.seq_len = M; g.kv_head_stride = M;
        if (chunks <= 1) { g.K = K16; g.V = V16; g.kv_chunks = 1; }
        else { g.K = ws.KVG; g.V = g.K; g.kv_chunks = chunks; g.kv_rows_per_chunk = M; g.kv_chunk_stride = (long long)(2 * hsz / 2); }
        int unit_rows = 256, per_cu = 2;
        wm_attention_geometry(g, &unit_rows, &per_cu);
        const int ntiles = (chunks < 1 ? 1 : chunks) * ntpc;
        const long slots = (long)per_cu * ncu, units = (long)((M + unit_rows - 1) / unit_rows) * heads;
        int best = 1; long best_cost = -1;
        for (int S = 1; S <= smax && S * 8 <= ntiles; ++S) {
          const long cost = ((units * S + slots - 1) / slots) * ((ntiles + S - 1) / S) + 6L * S;  // + partial write / read per slice
          if (best_cost < 0 || cost < best_cost) { best_cost = cost; best = S; }
        }
        return best;
      };
      const int nb = rank, nc = world - 1 - rank;  // remote chunks before / after the own one
      const int sa = pick(1, 2);
      const int sb = nb > 0 ? pick(nb, nc > 0 ? 3 : 6) : 0, sc = nc > 0 ? pick(nc, WM_ATTN_MAX_SPLITS - sa - sb) : 0;
      a.force_partial = 1;
      // (1) local keys, while the gather is in flight
      a.K = K16; a.V = V16; a.seq_len = M; a.kv_head_stride = M; a.kv_chunks = 1; a.kv_chunk_stride = 0; a.kv_rows_per_chunk = 0;
      a.kv_splits = sa; a.part_slot0 = 0;
      {
        ProfScope ps(h, 0, c.s);
        LCHK(c, wm_launch_attention(a, c.s));
      }
      LCHK(c, hipStreamWaitEvent(h->cstream, h->cfork, 0));
      st = comm_allgather(h, K16, KVG, 2 * hsz, h->cstream);
      if (st) return st;
      LCHK(c, hipEventRecord(h->cjoin, h->cstream));
      LCHK(c, hipStreamWaitEvent(c.s, h->cjoin, 0));
      // (2) remote keys: gathered chunks [0, rank) and (rank, world)
      ProfScope ps(h, 0, c.s);
      a.seq_len = M; a.kv_head_stride = M; a.kv_chunk_stride = (long long)(2 * hsz / 2); a.kv_rows_per_chunk = M;
      if (nb > 0) {
        a.K = KVG; a.V = KVG + hsz; a.kv_chunks = nb; a.kv_splits = sb; a.part_slot0 = sa; a.unit_hint = hint0 + hint_n; a.unit_stat = stat0 + 1;
        LCHK(c, wm_launch_attention(a, c.s));
      }
      if (nc > 0) {
        char* base = KVG + (size_t)(rank + 1) * 2 * hsz;
        a.K = base; a.V = base + hsz; a.kv_chunks = nc; a.kv_splits = sc; a.part_slot0 = sa + sb; a.unit_hint = hint0 + 2 * hint_n; a.unit_stat = stat0 + 2;
        LCHK(c, wm_launch_attention(a, c.s));
      }
      LCHK(c, wm_launch_attention_combine(a, sa + sb + sc, c.s));
    } else {
      if (sharded) {
        // K and V are adjacent: one all-gather of [K|V] per layer -> [world][2][H][M][64]
        char* KVG = ws.KVG;
        st = comm_allgather(h, K16, KVG, 2 * hsz, c.s);
        if (st) return st;
        a.K = KVG; a.V = KVG + hsz; a.seq_len = M; a.kv_head_stride = M; a.kv_chunks = d.world;
        a.kv_chunk_stride = (long long)(2 * hsz / 2); a.kv_rows_per_chunk = M;
      } else {
        a.K = K16; a.V = V16; a.seq_len = seq_len; a.kv_head_stride = M; a.kv_chunks = 1; a.kv_chunk_stride = 0; a.kv_rows_per_chunk = 0;
      }
      if (general_only) { a.unit_flags = nullptr; a.unit_hint = nullptr; a.unit_stat = nullptr; }
      ProfScope ps(h, is_global ? 0 : 1, c.s);
      LCHK(c, wm_launch_attention(a, c.s));
    }
  }
  {
    WmGemmArgs ex;
    memset(&ex, 0, sizeof(ex));
    fuse_args(ex, w.norm2);
    bool fused = false;
    st = gemm(c, dt, WM_EPI_RESID, O16, D, w.proj.w, D, X, D, w.proj.b, w.ls1, M, D, D, &ex, -1, &fused);
    if (st) return st;
    if (!fused) {
      ln.w = w.norm2.w; ln.b = w.norm2.b;
      st = layernorm(c, ln);
      if (st) return st;
    }
  }
  const int Hd = c.h->cfg.mlp_ratio * D;
  st = gemm(c, dt, WM_EPI_GELU_T16, A16, D, w.fc1.w, D, H16, Hd, w.fc1.b, nullptr, M, Hd, D);
  if (st) return st;
  WmGemmArgs ex;
  memset(&ex, 0, sizeof(ex));
  ex.C2 = tap_half; ex.ldc2 = 2 * D;
  bool fused = false;
  if (next_norm1) fuse_args(ex, *next_norm1);
  st = gemm(c, dt, WM_EPI_RESID, H16, Hd, w.fc2.w, Hd, X, D, w.fc2.b, w.ls2, M, D, Hd, &ex, -1, &fused);
  if (ln1_ready) *ln1_ready = fused;
  return st;
}

wm_status linear32(Ctx& c, const float* X, int ldx, const Lin32& w, float* Y, int ldy, int M, int pre, int post,
                   const float* gamma = nullptr, int accumulate = 0) {
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

// ---- token-conv: Conv2d(3x3, pad 1, no bias) o ConvTranspose2d(kernel = stride = k) composed at the token resolution (WmGemmArgs::tc_k)
// For output phase (a, b) of token (i, j) the 3x3 taps land in at most two token rows and two token columns:
//   rn[(k i + a, k j + b)] = sum over neighbours (di, dj) of M[a, b, di, dj] p[i + di][j + dj]  +  (sum over taps inside the image of W_rn[tap]) b_ct
//   M[a, b, di, dj] = sum over taps (dy, dx) with floor((a + dy) / k) = di, floor((b + dx) / k) = dj of W_rn[tap] W_ct[(a + dy) mod k][(b + dx) mod k]
// 36 (phase, neighbour) matrices for k = 4, 16 for k = 2, instead of k^2 x 9 tap products per token: 4.4x / 2.7x fewer flops than ConvTranspose
// GEMM + 3x3 conv, no ConvTranspose output tensor, one rounding of the combined weight instead of two operand roundings.
// wct: torch ConvTranspose2d weight [Cin][Cm][k][k], bct [Cm], wrn: torch Conv2d weight [F][Cm][3][3] (host fp32).  F must be 256.
static hipError_t build_tconv(int dt, int k, int Cin, int Cm, int F_, const float* wct, const float* bct, const float* wrn, TconvPack& out, hipStream_t s) {
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
static hipError_t build_tapfold(int dt, int nh, int oc, int K, int Kp, const float* const* Wh, const float* const* bh, const float* const* gamma,
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
void* tap_front_dst(const wm_handle* h, const Dims& d, const HeadBufs& hb, int i, int v0) {
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

// rn = tconv(tokens): tokens16 [n][gh][gw][Cin] (16-bit) -> out fp32 [n][k gh][k gw][256]
static hipError_t launch_tconv(const TconvPack& t, int dt, const void* tokens16, float* out, int n, int gh, int gw, const void* zero16, hipStream_t s) {
  WmGemmArgs g;
  memset(&g, 0, sizeof(g));
  g.A = tokens16; g.W = t.w16; g.C = out; g.bias = t.bias_rep; g.M = n * gh * gw; g.N = t.k * t.k * 256; g.K = 4 * t.cin; g.lda = t.cin; g.ldw = 4 * t.cin; g.ldc = 256;
  g.dtype = dt; g.epi = WM_EPI_CONV; g.cv_h = gh; g.cv_w = gw; g.cv_cin = t.cin; g.cv_zero = zero16; g.tc_k = t.k;
  memcpy(g.tc_list, t.list, sizeof(g.tc_list));
  hipError_t e = wm_launch_gemm(g, s);
  if (e != hipSuccess) return e;
  return wm_launch_tconv_border(out, t.bmiss, n, t.k * gh, t.k * gw, 256, s);
}

// the geometry of a conv launch; the caller then sets, by field name, whatever else differs from zero (residuals, ReLUs, 16-bit forms, fused resize)
WmConvArgs conv_args(const float* x, float* y, int N, int Hi, int Wi, int ksize, int stride, int pad) {
  WmConvArgs a;
  memset(&a, 0, sizeof(a));
  a.x = x; a.y = y; a.N = N; a.Hi = Hi; a.Wi = Wi; a.ksize = ksize; a.stride = stride; a.pad = pad;
  return a;
}

// a.up_hs > 0: x is [N][up_hs][up_ws][Cin] and the conv runs on its align_corners bilinear resize to (Hi, Wi)
// (+ position tables), fused into the 3x3 halo kernel's input staging.
// The weight, bias, channel counts, output size and operand type are filled in here.
wm_status conv(Ctx& c, const ConvW& w, WmConvArgs a, bool* out16 = nullptr) {
  a.w = w.w16; a.bias = w.bias; a.Cin = w.cin; a.Cout = w.cout; a.dtype = c.hdt;
  a.Ho = (a.Hi + 2 * a.pad - a.ksize) / a.stride + 1; a.Wo = (a.Wi + 2 * a.pad - a.ksize) / a.stride + 1;
  if (out16) {  // the caller can take y as a 16-bit tensor (its only consumer rounds it to the operand type anyway): granted when the kernel can
    *out16 = wm_conv3x3_out16_ok(a);
    a.out16 = *out16 ? 1 : 0;
  }
  // timing kinds by kernel instantiation: the F -> F 3x3 convs of the two large pyramid levels, output_conv1 with its fused
  // resize; everything else (small levels, 1x1, stride 2) under 3
  const bool pyr = a.ksize == 3 && a.stride == 1 && a.up_hs == 0 && a.Cin == a.Cout && a.Cin >= 128;
  const int kind = a.up_hs > 0 ? 10 : pyr && a.Hi == 4 * c.d.gh ? 8 : pyr && a.Hi == 2 * c.d.gh ? 9 : 3;
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
wm_status rcu(Ctx& c, const ConvW (&w)[2], const float* x, const float* extra, float* tmp, float* y, int N, int Hh, int Ww, bool* y16 = nullptr) {
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
wm_status out_conv(Ctx& c, const ConvW& w, const float* x2, bool x2_is_16, float* y, int N, int Hh, int Ww, int F_, bool y16 = false) {
  if (!x2_is_16) return y16 ? fail(c.h, WM_ERR_STATE, "out_conv: 16-bit output needs the 16-bit input") : conv(c, w, conv_args(x2, y, N, Hh, Ww, 1, 1, 0));
  return gemm(c, c.hdt, y16 ? WM_EPI_T16 : WM_EPI_F32, x2, F_, w.w16, F_, y, F_, w.bias, nullptr, N * Hh * Ww, F_, F_, nullptr, 3);
}

// DPTHead (dense_head.py:107-295) for views [v0, v0+n) of this rank: head `id` (its weights) in workspace slot `slot` (its buffers)
wm_status dpt_head(Ctx& c, int id, int F_, int out_dim, int act, float* out_attr, float* out_conf,
                   const float* img, const wm_outputs* out, int first_view, int slot, bool front_done = false) {
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
  float* S0 = hb.s[0]; float* S1 = hb.s[1]; float* S2 = hb.s[2]; float* S3 = hb.s[3];
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
          ProfScope ps(h, i == 0 ? 8 : 3, c.s);
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
      int k = 0;
      for (float* b : {S0, S1, S2, S3}) if (b != cur) others[k++] = b;
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
    {
      int k = 0;
      for (float* b : {S0, S1, S2, S3}) if (b != cur) others[k++] = b;
    }
    if (up1_gather) {
      void* Y1 = others[1];
      if (comp) st = gemm(c, c.hdt, WM_EPI_T16, cur, F_, comp->w16, F_, Y1, 9 * Co1, comp->bias, nullptr, n * Hs[0] * Ws[0], 9 * Co1, F_, nullptr, 10);
      else st = gemm(c, c.hdt, WM_EPI_T16, cur, F_, w.oc1_tap, F_, Y1, 9 * Co1, nullptr, nullptr, n * Hs[0] * Ws[0], 9 * Co1, F_, nullptr, 10);
      if (!st) {
        ProfScope ps(h, 10, c.s);
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
      ProfScope ps(h, 11, c.s);
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

wm_status forward_impl(wm_handle* h, const float* img, int n, int first_view, int nt, int H, int W_, const float* pose7,
                       const float* depth, const float* ray4, const int32_t* flags, const wm_outputs* out, hipStream_t s) {
  if (!h || !img || !out) return WM_ERR_INVALID;
  if (!h->finalized) return fail(h, WM_ERR_STATE, "weights not finalized");
  const wm_config& cf = h->cfg;
  if (n <= 0 || nt < n || nt % n) return fail(h, WM_ERR_INVALID, "n_total must be a positive multiple of n_local");
  if (H % cf.patch_size || W_ % cf.patch_size) return fail(h, WM_ERR_INVALID, "H and W must be multiples of patch_size");
  if (nt / n > 1 && (h->comm.kind == 0 || h->comm.world != nt / n)) return fail(h, WM_ERR_COMM, "communicator world size mismatch");
  HIPCHK(h, hipSetDevice(h->device));
  Ctx c{h, make_dims(h, n, nt, H, W_), s, cf.backbone_dtype, cf.head_dtype};
  const Dims& d = c.d;
  // no allocation, no host-side table building and no synchronisation in the forward: the workspace must exist
  if (!(h->plan_n == d.n && h->plan_nt == d.nt && h->plan_H == d.H && h->plan_W == d.W))
    return fail(h, WM_ERR_STATE, "no workspace for this shape: call wm_reserve(h, n_local, n_total, H, W) first (and again after loading weights)");
  wm_status st = WM_OK;
  for (int k = 0; k < wm_handle::NKIND; ++k) h->ev_used[k] = 0;
  ProfScope whole(h, 4, s);
  const Model& m = h->m;
  const Workspace& ws = h->ws;
  HIPCHK(h, hipMemsetAsync(ws.ZERO256, 0, 256, s));
  const int D = d.D;
  float* Xd = ws.Xd;
  float* Xv = ws.Xv;
  void* A16 = ws.A16;

  // ---- a3/a4: normalise + patchify + DINOv2 encoder (vision_transformer.py:209-266)
  LCHK(c, wm_launch_im2col(img, A16, n, 3, H, W_, cf.patch_size, d.kpad_patch, 1, c.bdt, s));
  {
    WmGemmArgs ex;
    memset(&ex, 0, sizeof(ex));
    ex.rows_per_group = d.hw; ex.out_group = d.Td; ex.out_off = 1 + d.R; ex.add = ws.dino_pos + D;
    st = gemm(c, c.bdt, WM_EPI_ROWMAP_ADD, A16, d.kpad_patch, m.patch_proj.w, d.kpad_patch, Xd, D, m.patch_proj.b, nullptr, n * d.hw, D, d.kpad_patch, &ex);
    if (st) return st;
  }
  LCHK(c, wm_launch_dino_tokens(nullptr, m.cls_token, m.register_tokens, ws.dino_pos, Xd, n, d.hw, d.R, D, s));
  {
    bool ln1 = false;
    for (int i = 0; i < cf.dino_depth; ++i) {
      const Norm* nxt = i + 1 < cf.dino_depth ? &m.dino[i + 1].norm1 : nullptr;
      st = backbone_block(c, m.dino[i], Xd, d.Md, d.Td, cf.dino_heads, 1e-6f, false, d.Td, 0, false, nullptr, ln1, nxt, &ln1);
      if (st) return st;
    }
  }
  // final LN, patch tokens only, straight into the multi-view token buffer
  {
    WmLnArgs ln{};
    ln.x = Xd; ln.ld_in = D; ln.y = Xv; ln.ld_out = D; ln.w = m.dino_norm.w; ln.b = m.dino_norm.b; ln.D = D; ln.eps = 1e-6f;
    ln.groups = n; ln.rows_per_group = d.hw; ln.in_group = d.Td; ln.in_off = 1 + d.R; ln.out_group = d.P; ln.out_off = d.psi; ln.out_f32 = 1;
    st = layernorm(c, ln);
    if (st) return st;
  }

  // ---- a5: special + prior tokens (visual_transformer.py:285-295,343-371)
  const float* pose_tok = nullptr; const float* ray_tok = nullptr;
  if (cf.enable_cond) {
    float* pin = ws.pr_in; float* ph = ws.pr_h;
    if (flags && flags[0] == 1 && pose7) {
      LCHK(c, hipMemcpy2DAsync(pin, 8 * 4, pose7, 7 * 4, 7 * 4, n, hipMemcpyDeviceToDevice, s));
      st = linear32(c, pin, 8, m.pose_embed[0], ph, D, n, 0, 1);
      if (st) return st;
      st = linear32(c, ph, D, m.pose_embed[1], ws.pose_tok, D, n, 0, 0);
      if (st) return st;
      pose_tok = ws.pose_tok;
    }
    if (flags && flags[2] == 1 && ray4) {
      st = linear32(c, ray4, 4, m.ray_embed[0], ph, D, n, 0, 1);
      if (st) return st;
      st = linear32(c, ph, D, m.ray_embed[1], ws.ray_tok, D, n, 0, 0);
      if (st) return st;
      ray_tok = ws.ray_tok;
    }
    if (flags && flags[1] == 1 && depth) {  // PatchEmbed_Mlp (patch_embed.py:79-93): unshuffle -> fc1 -> GELU -> fc2, added to patches
      LCHK(c, wm_launch_im2col(depth, A16, n, 1, H, W_, cf.patch_size, d.kpad_depth, 0, c.bdt, s));
      void* H16 = ws.H16;
      st = gemm(c, c.bdt, WM_EPI_GELU_T16, A16, d.kpad_depth, m.depth_fc1.w, d.kpad_depth, H16, 4 * D, m.depth_fc1.b, nullptr, n * d.hw, 4 * D, d.kpad_depth);
      if (st) return st;
      WmGemmArgs ex;
      memset(&ex, 0, sizeof(ex));
      ex.rows_per_group = d.hw; ex.out_group = d.P; ex.out_off = d.psi; ex.accumulate = 1;
      st = gemm(c, c.bdt, WM_EPI_ROWMAP_ADD, H16, 4 * D, m.depth_fc2.w, 4 * D, Xv, D, m.depth_fc2.b, nullptr, n * d.hw, D, 4 * D, &ex);
      if (st) return st;
    }
  }
  LCHK(c, wm_launch_vgt_special(Xv, m.cam_token, m.reg_token, pose_tok, ray_tok, n, d.P, d.R, D, cf.enable_cond, first_view, s));

  // ---- a7-a10: 24 x (frame block, global block) + taps (visual_transformer.py:309-339)
  int tap_i = 0;
  bool vgt_ln1 = false;   // A16 already holds the coming block's norm1(X): the previous block's fc2 epilogue wrote it
  for (int i = 0; i < cf.depth; ++i) {
    const bool is_tap = tap_i < 4 && i == cf.intermediate_idxs[tap_i];
    float* tap = is_tap ? ws.tap[tap_i] : nullptr;
    // (frame and global blocks alternate on the same token buffer: each block's fc2 epilogue computes the next block's norm1)
    const Norm* fnext = i + 1 < cf.depth ? &m.frame[i + 1].norm1 : nullptr;
    st = backbone_block(c, m.frame[i], Xv, d.Mv, d.P, cf.num_heads, 1e-5f, true, d.P, d.psi, false, tap, vgt_ln1, &m.global[i].norm1, &vgt_ln1);
    if (st) return st;
    st = backbone_block(c, m.global[i], Xv, d.Mv, d.Mv, cf.num_heads, 1e-5f, true, d.P, d.psi, true, tap ? tap + D : nullptr, vgt_ln1, fnext, &vgt_ln1);
    if (st) return st;
    if (is_tap) {
      if (out->taps[tap_i]) LCHK(c, hipMemcpyAsync(out->taps[tap_i], tap, (size_t)d.Mv * 2 * D * 4, hipMemcpyDeviceToDevice, s));
      ++tap_i;
    }
  }

  // fallback statistics of the fast attention kernels -> pinned host mirror (read by the NEXT forwards' launch policy; no synchronisation)
  if (h->att_stat_host) LCHK(c, hipMemcpyAsync(h->att_stat_host, ws.ATT_STAT, (size_t)h->att_stat_n * 4, hipMemcpyDeviceToHost, s));

  // The camera head and the DPT heads are independent of each other: each runs on one of the handle's own queues, forked from and
  // joined back to the caller's stream (-1.15 ms per forward at 8 x 518^2, -5 ms at 32 views: the HBM-bound camera head and the under-filled small DPT
  // levels run beside the MFMA-bound convs).  Tuning heads_concurrent = 0 keeps one queue.
  // History: round 1 saw sparse wrong lanes with several queues active and fenced this off; round 2 traced it to packed-fp32 VALU
  // instructions (compiler-generated v_pk_mul_f32 / v_pk_fma_f32, op_sel forms) dropping one half's result in 16-lane groups when a
  // kernel of another kind shares the SIMD from another queue — reproduced without torch on the ROCm 7.2 runtime with the library's own
  // kernels (tools/micro/splat_hazard_repro.cpp, profiles/r02_multiqueue_hazard.md), never with one queue, never without packed fp32.
  // No kernel outside the GELU instantiations of gemm.hip contains a packed-fp32 instruction any more (-fno-slp-vectorize,
  // WM_NO_PACKED_FP32 in wm_common.h; held by tests/test_kernel_resources_cpu.py, which disassembles every object), and those
  // GELU GEMMs of the backbone have finished before this fork.  tools/stress_concurrent_heads.py: 4 900 concurrent forwards (C2, C3, C5 flag set) bit-identical
  // to the serial one.
  const bool serial = wm_tune(WM_TUNE_HEADS_CONC, 1) == 0 || h->prof;
  if (!h->hfork) LCHK(c, hipEventCreateWithFlags(&h->hfork, hipEventDisableTiming));
  if (!serial) LCHK(c, hipEventRecord(h->hfork, s));
  // ---- a11-a12: camera head.  864 MB of fp32 weights streamed 4 times for <= 64 rows: HBM-bound (1.3 ms at 8 views), so it runs
  // on its own queue BESIDE the MFMA-bound DPT heads (which do not depend on it, except the Gaussian head's splat assembly).
  bool cam_async = false;
  if (cf.enable_cam && out->camera_params) {
    Ctx cc = c;
    if (!serial) {
      if (!h->camstream) {
        LCHK(c, hipStreamCreateWithFlags(&h->camstream, hipStreamNonBlocking));
        LCHK(c, hipEventCreateWithFlags(&h->camjoin, hipEventDisableTiming));
      }
      cc.s = h->camstream;
      LCHK(c, hipStreamWaitEvent(cc.s, h->hfork, 0));
      cam_async = true;
    }
    st = camera_head(cc, ws.cam_params);
    if (st) return st;
    LCHK(c, hipMemcpyAsync(out->camera_params, ws.cam_params, (size_t)nt * 9 * 4, hipMemcpyDeviceToDevice, cc.s));
    if (out->camera_poses && out->camera_intrs)
      LCHK(c, wm_launch_cam_matrices(ws.cam_params, out->camera_poses, out->camera_intrs, nt, H, W_, cc.s));
    if (cam_async) LCHK(c, hipEventRecord(h->camjoin, cc.s));
  }
  // ---- a13: DPT heads (worldmirror.py:74-98): independent of each other; one per queue unless tuning heads_concurrent = 0 (see above).
  {
    struct HeadJob { int id; int F; int od; int act; float* attr; float* conf; };   // id: which head (HeadId); its index in jobs is its workspace slot
    std::vector<HeadJob> jobs;
    if (cf.enable_depth && out->depth && out->depth_conf) jobs.push_back({HD_DEPTH, cf.dpt_features, 2, WM_ACT_EXP, out->depth, out->depth_conf});
    if (cf.enable_pts && out->pts3d && out->pts3d_conf) jobs.push_back({HD_PTS, cf.dpt_features, 4, WM_ACT_INV_LOG, out->pts3d, out->pts3d_conf});
    if (cf.enable_norm && out->normals && out->normals_conf) jobs.push_back({HD_NORM, cf.dpt_features, 4, WM_ACT_NORM, out->normals, out->normals_conf});
    if (cf.enable_gs && out->gs_depth && out->gs_depth_conf) {
      if (out->splat_means && !(out->splat_quats && out->splat_scales && out->splat_opacities && out->splat_sh && out->splat_weights))
        return fail(h, WM_ERR_INVALID, "splat outputs must be given together");
      if (out->splat_means && !(cf.enable_cam && out->camera_params)) return fail(h, WM_ERR_INVALID, "splats need the camera head");
      jobs.push_back({HD_GS, cf.gs_dim, 2, WM_ACT_EXP, out->gs_depth, out->gs_depth_conf});
    }
    // Round 4: the LAST head runs on the caller's stream itself and only the others fork.  HIP multiplexes streams onto four hardware
    // queues: with every head on a stream of its own (three heads + the camera head + the caller's idle stream) two DPT heads shared
    // a hardware queue and ran one after the other — the kernel trace of a timed forward showed one head done after 7.5 ms and the other
    // two, serialised, after 12.3 ms (profiles/r04_head_phase_queues.md).  Side heads are enqueued first, the caller's stream joins them
    // only behind its own head's launches.
    // The heads' front — LayerNorm of each tap and its 1x1 projection — once for all heads on the caller's stream (tuning tap_shared = 0: every
    // head normalises and projects for itself).  Taken when the folded weights exist (wm_reserve: two or more heads, in range) and the call
    // runs exactly the group's heads, whose order numbers the workspace slots.
    bool front = wm_tune(WM_TUNE_TAP_SHARED, 1) != 0 && h->tapfold.valid && (size_t)h->tapfold.nh == jobs.size();
    for (size_t k = 0; front && k < jobs.size(); ++k) front = h->tapfold.heads[k] == jobs[k].id;
    if (front) {
      st = tap_front(c);
      if (st) return st;
      if (!serial) {
        if (!h->hfront) LCHK(c, hipEventCreateWithFlags(&h->hfront, hipEventDisableTiming));
        LCHK(c, hipEventRecord(h->hfront, s));
      }
    }
    const size_t main_k = jobs.empty() || wm_tune(WM_TUNE_HEADS_MAIN, 1) == 0 ? (size_t)-1 : jobs.size() - 1;   // (tuning heads_main = 0: every head forks, round 3's form — A/B)
    auto run_head = [&](size_t k, hipStream_t hs) -> wm_status {
      Ctx hc = c;
      hc.s = hs;
      if (jobs[k].id == HD_GS && cam_async) LCHK(c, hipStreamWaitEvent(hs, h->camjoin, 0));  // the splats are unprojected with the predicted cameras
      return dpt_head(hc, jobs[k].id, jobs[k].F, jobs[k].od, jobs[k].act, jobs[k].attr, jobs[k].conf, img, out, first_view, (int)k, front);
    };
    const bool fork_heads = !serial && (jobs.size() > 1 || cam_async);
    for (size_t k = 0; k < jobs.size(); ++k) {
      if (fork_heads && k == main_k) continue;
      hipStream_t hs = s;
      if (fork_heads) {
        if (!h->hstream[k]) LCHK(c, hipStreamCreateWithFlags(&h->hstream[k], hipStreamNonBlocking));
        if (!h->hjoin[k]) LCHK(c, hipEventCreateWithFlags(&h->hjoin[k], hipEventDisableTiming));
        hs = h->hstream[k];
        LCHK(c, hipStreamWaitEvent(hs, front ? h->hfront : h->hfork, 0));
      }
      st = run_head(k, hs);
      if (st) return st;
      if (hs != s) LCHK(c, hipEventRecord(h->hjoin[k], hs));
    }
    if (fork_heads && !jobs.empty()) {
      if (main_k != (size_t)-1) {
        st = run_head(main_k, s);
        if (st) return st;
      }
      for (size_t k = 0; k < jobs.size(); ++k)
        if (k != main_k) LCHK(c, hipStreamWaitEvent(s, h->hjoin[k], 0));
    }
  }
  if (cam_async) LCHK(c, hipStreamWaitEvent(s, h->camjoin, 0));
  return WM_OK;
}

}  // namespace

extern "C" wm_status wm_forward(wm_handle* h, const float* img, int N, int H, int W, const float* pose7, const float* depth,
                                const float* ray4, const int32_t cond_flags[3], const wm_outputs* out, void* stream) {
  return forward_impl(h, img, N, 0, N, H, W, pose7, depth, ray4, cond_flags, out, (hipStream_t)stream);
}

extern "C" wm_status wm_forward_sharded(wm_handle* h, const float* img, int n_local, int first_view, int n_total, int H, int W,
                                        const float* pose7, const float* depth, const float* ray4, const int32_t cond_flags[3],
                                        const wm_outputs* out, void* stream) {
  return forward_impl(h, img, n_local, first_view, n_total, H, W, pose7, depth, ray4, cond_flags, out, (hipStream_t)stream);
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

// ====================================================================================== communicator
extern "C" wm_status wm_rccl_unique_id(uint8_t id[WM_RCCL_ID_BYTES]) {
  static_assert(sizeof(ncclUniqueId) <= WM_RCCL_ID_BYTES, "id buffer too small");
  ncclUniqueId u;
  if (ncclGetUniqueId(&u) != ncclSuccess) return WM_ERR_COMM;
  memset(id, 0, WM_RCCL_ID_BYTES);
  memcpy(id, &u, sizeof(u));
  return WM_OK;
}

extern "C" wm_status wm_comm_init_rccl(wm_handle* h, const uint8_t id[WM_RCCL_ID_BYTES], int rank, int world) {
  if (!h || !id || world < 1 || rank < 0 || rank >= world) return WM_ERR_INVALID;
  HIPCHK(h, hipSetDevice(h->device));
  ncclUniqueId u;
  memcpy(&u, id, sizeof(u));
  if (ncclCommInitRank(&h->comm.nccl, world, u, rank) != ncclSuccess) return fail(h, WM_ERR_COMM, "ncclCommInitRank failed");
  h->comm.kind = 1; h->comm.rank = rank; h->comm.world = world;
  return WM_OK;
}

extern "C" wm_local_group* wm_local_group_create(int world) {
  wm_local_group* g = new wm_local_group();
  g->world = world;
  g->recv.assign(world, nullptr);
  pthread_barrier_init(&g->bar, nullptr, world);
  return g;
}
extern "C" void wm_local_group_destroy(wm_local_group* g) {
  if (!g) return;
  pthread_barrier_destroy(&g->bar);
  delete g;
}
extern "C" wm_status wm_comm_init_local(wm_handle* h, wm_local_group* g, int rank) {
  if (!h || !g || rank < 0 || rank >= g->world) return WM_ERR_INVALID;
  h->comm.kind = 2; h->comm.rank = rank; h->comm.world = g->world; h->comm.grp = g;
  return WM_OK;
}

extern "C" wm_status wm_allgather(wm_handle* h, const void* send, void* recv, size_t bytes_per_rank, void* stream) {
  if (!h || !send || !recv || bytes_per_rank == 0) return WM_ERR_INVALID;
  return comm_allgather(h, send, recv, bytes_per_rank, (hipStream_t)stream);
}

// ====================================================================================== profiling
extern "C" wm_status wm_profile_enable(wm_handle* h, int on) {
  if (!h) return WM_ERR_INVALID;
  h->prof = on != 0;
  return WM_OK;
}
extern "C" wm_status wm_profile_read(wm_handle* h, int kind, double* total_ms, int64_t* launches) {
  if (!h || kind < 0 || kind >= wm_handle::NKIND) return WM_ERR_INVALID;
  double tot = 0;
  for (size_t i = 0; i < h->ev_used[kind]; ++i) {
    float ms = 0;
    HIPCHK(h, hipEventSynchronize(h->ev[kind][i].b));
    HIPCHK(h, hipEventElapsedTime(&ms, h->ev[kind][i].a, h->ev[kind][i].b));
    tot += ms;
  }
  if (total_ms) *total_ms = tot;
  if (launches) *launches = (int64_t)h->ev_used[kind];
  return WM_OK;
}

// ====================================================================================== operator-level entry points
// Only the two that run the forward's own building blocks and need this file's local types; every other wm_op_* is in wm_api_ops.cpp.
// Conv2d(Cm, 256, 3, padding=1, bias=False)(ConvTranspose2d(Cin, Cm, k, stride=k)(tokens)) composed at the token resolution (build_tconv):
// tokens16 [N][gh][gw][Cin] 16-bit device; wct [Cin][Cm][k][k], bct [Cm], wrn [256][Cm][3][3]: HOST fp32 in torch's layouts; out fp32 [N][k gh][k gw][256]
extern "C" wm_status wm_op_tconv(int dtype, const void* tokens16, const float* wct, const float* bct, const float* wrn, float* out, int N, int gh, int gw,
                                 int k, int Cin, int Cm, const void* zero16, void* stream) {
  if (!tokens16 || !wct || !bct || !wrn || !out || !zero16) return WM_ERR_INVALID;
  TconvPack t;
  hipStream_t s = (hipStream_t)stream;
  if (build_tconv(dtype, k, Cin, Cm, 256, wct, bct, wrn, t, s) != hipSuccess) return WM_ERR_HIP;
  const hipError_t e = launch_tconv(t, dtype, tokens16, out, N, gh, gw, zero16, s);
  (void)hipStreamSynchronize(s);
  free_tconv(t);
  return e == hipSuccess ? WM_OK : WM_ERR_HIP;
}
// The DPT heads' tap front for one tap (dense_head.py:53,204-208), both forms the forward has: shared = 0 every head normalises the tap with its
// own affine and projects it; shared = 1 one LayerNorm without affine and one GEMM over the heads' folded weights (build_tapfold), unless a folded
// weight leaves the operand type's range — then the direct form runs (*ran_shared tells).  Host fp32 weights, device tap / pos / outputs.
extern "C" wm_status wm_op_dpt_tap_front(int dtype, const float* tap, int n, int P, int psi, int hw, int D2, int nheads, int oc,
                                         const float* const* norm_w, const float* const* norm_b, const float* const* proj_w,
                                         const float* const* proj_b, const float* pos, int out16, int shared, void* const* out, int* ran_shared,
                                         void* stream) {
  if (!tap || !norm_w || !norm_b || !proj_w || !proj_b || !out || n <= 0 || hw <= 0 || psi < 0 || P < psi + hw || D2 <= 0 || D2 % 64 || nheads < 1 ||
      nheads > 4 || oc <= 0 || (oc & 3) || (dtype != WM_DT_BF16 && dtype != WM_DT_F16))
    return WM_ERR_INVALID;
  for (int k = 0; k < nheads; ++k)
    if (!norm_w[k] || !norm_b[k] || !proj_w[k] || !proj_b[k] || !out[k]) return WM_ERR_INVALID;
  hipStream_t s = (hipStream_t)stream;
  wm_handle tmp;
  Ctx c{&tmp, Dims(), s, dtype, dtype};
  if (ran_shared) *ran_shared = 0;
  std::vector<void*> dev;
  auto dalloc = [&](size_t bytes) -> void* { void* q = nullptr; if (hipMalloc(&q, bytes) != hipSuccess) return nullptr; dev.push_back(q); return q; };
  auto finish = [&](wm_status st) {
    (void)hipStreamSynchronize(s);
    for (void* q : dev) (void)hipFree(q);
    return st;
  };
  void* xhat = dalloc((size_t)n * hw * D2 * 2);
  if (!xhat) return finish(WM_ERR_HIP);
  if (shared) {
    void* w16 = nullptr; float* bias = nullptr; bool in_range = false;
    if (build_tapfold(dtype, nheads, oc, D2, D2, proj_w, proj_b, norm_w, norm_b, &w16, &bias, &in_range) != hipSuccess) return finish(WM_ERR_HIP);
    if (in_range) {
      dev.push_back(w16); dev.push_back(bias);
      if (ran_shared) *ran_shared = 1;
      return finish(tap_front_one(c, tap, xhat, w16, bias, pos, nheads, oc, out16, out, n, hw, P, psi, D2));
    }
  }
  for (int k = 0; k < nheads; ++k) {   // the direct form, as dpt_head runs it
    float* gw = (float*)dalloc((size_t)D2 * 4); float* gb = (float*)dalloc((size_t)D2 * 4); float* pb = (float*)dalloc((size_t)oc * 4);
    void* w16 = dalloc((size_t)oc * D2 * 2);
    if (!gw || !gb || !pb || !w16) return finish(WM_ERR_HIP);
    std::vector<uint16_t> r((size_t)oc * D2);
    for (size_t i = 0; i < r.size(); ++i) r[i] = h_to16(proj_w[k][i], dtype);
    if (hipMemcpy(gw, norm_w[k], (size_t)D2 * 4, hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(gb, norm_b[k], (size_t)D2 * 4, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(pb, proj_b[k], (size_t)oc * 4, hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(w16, r.data(), r.size() * 2, hipMemcpyHostToDevice) != hipSuccess)
      return finish(WM_ERR_HIP);
    WmLnArgs ln{};
    ln.x = tap; ln.ld_in = D2; ln.y = xhat; ln.ld_out = D2; ln.w = gw; ln.b = gb; ln.D = D2; ln.eps = 1e-5f;
    ln.groups = n; ln.rows_per_group = hw; ln.in_group = P; ln.in_off = psi; ln.out_group = hw; ln.dtype = dtype;
    wm_status st = layernorm(c, ln);
    if (st) return finish(st);
    WmGemmArgs ex;
    memset(&ex, 0, sizeof(ex));
    ex.rows_per_group = hw; ex.out_group = hw; ex.out_off = 0; ex.add = pos; ex.out16 = out16;
    st = gemm(c, dtype, WM_EPI_ROWMAP_ADD, xhat, D2, w16, D2, out[k], oc, pb, nullptr, n * hw, oc, D2, &ex);
    if (st) return finish(st);
    if (hipStreamSynchronize(s) != hipSuccess) return finish(WM_ERR_HIP);   // xhat is reused by the next head
  }
  return finish(WM_OK);
}
