// Internal to the host orchestrator (never installed): the handle, the weight store's and the bound model's types, and the functions that
// cross its translation units — wm_weights.cpp, wm_compose.cpp, wm_plan.cpp, wm_comm.cpp, wm_backbone.cpp, wm_heads.cpp, wm_model.cpp and
// the two operator entries of wm_api_ops.cpp that run the forward's own building blocks.  Everything here but the two C-ABI handle types is in
// the hidden namespace wm_host: the library's dynamic symbol table holds the entries of include/wm_hip.h only.
#pragma once
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

namespace wm_host __attribute__((visibility("hidden"))) {

inline int ru(int x, int m) { return (x + m - 1) / m * m; }

uint16_t h_to16(float f, int dt);   // round to nearest even to bf16 / f16 (wm_weights.cpp)

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

// the composed ConvTranspose -> 3x3 conv of a DPT head level (build_tconv, wm_compose.cpp)
struct TconvPack {
  void* w16 = nullptr;        // [k^2 * 256][4 * Cin] 16-bit: row (phase, co), the phase's neighbour matrices side by side
  float* bias_rep = nullptr;  // [k^2][256]: (sum_tap W_rn[tap]) b_ct, once per phase
  float* bmiss = nullptr;     // [9][256]: W_rn[tap] b_ct (wm_launch_tconv_border)
  unsigned list[16] = {0};
  int k = 0, cin = 0;
};
void free_tconv(TconvPack& t);
hipError_t build_tconv(int dt, int k, int Cin, int Cm, int F_, const float* wct, const float* bct, const float* wrn, TconvPack& out, hipStream_t s);
// refinenet1.out_conv (1x1) composed into the nine tap matrices of output_conv1 (upconv.hip): the tap GEMM then reads the last fusion block's
// 16-bit tensor directly — W[tap][co][ci] = sum_c W_oc1[co][c][tap] W_out[c][ci], bias[tap][co] = sum_c W_oc1[co][c][tap] b_out[c] (build_up1comp)
struct Up1Comp {
  void* w16 = nullptr;     // [9 Co][F] 16-bit
  float* bias = nullptr;   // [9 Co]
  int co = 0;
};
void free_up1comp(Up1Comp& u);

// The DPT heads' tap front shared between heads (tuning tap_shared): LayerNorm(2D) -> projects.i (dense_head.py:53,204-208) with each head's
// LayerNorm affine folded into its projection, W'_h = W_h diag(gamma_h), b'_h = b_h + W_h beta_h, the heads' rows one under the other: all heads
// then read the SAME normalised tap and one GEMM per tap serves them all (build_tapfold, wm_compose.cpp)
struct TapFold {
  void* w16[4] = {nullptr, nullptr, nullptr, nullptr};      // per tap [nh * oc_i][Kp] 16-bit
  float* bias[4] = {nullptr, nullptr, nullptr, nullptr};    // per tap [nh * oc_i]
  int heads[4] = {0, 0, 0, 0}, nh = 0;                      // the group's heads (HeadId), in the order of their row blocks
  bool valid = false;                                       // false: no group, or a folded weight left the operand type's range (direct form)
};
void free_tapfold(TapFold& t);
// one tap: W[h] [oc][K], b[h] [oc], gamma[h], beta[h] [K] (host fp32) -> w16 [nh oc][Kp], bias [nh oc] on the device; *in_range = false (and nothing
// allocated) when a folded weight or bias is not finite, or a weight exceeds the f16 maximum for f16 operands
hipError_t build_tapfold(int dt, int nh, int oc, int K, int Kp, const float* const* Wh, const float* const* bh, const float* const* gamma,
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

// timing kinds of wm_profile_read: the values are those documented in include/wm_hip.h and read by bench.py
enum ProfKind {
  PK_ATTN_GLOBAL = 0,   // global attention
  PK_ATTN_LOCAL = 1,    // frame + DINO attention
  PK_GEMM = 2,          // GEMM, epilogues other than the three below
  PK_CONV = 3,          // DPT convs other than those below
  PK_FORWARD = 4,       // the whole forward
  PK_GEMM_QKV = 5,
  PK_GEMM_RESID = 6,    // proj, fc2
  PK_GEMM_GELU = 7,     // fc1
  PK_CONV_4X = 8,       // 3x3 convs F -> F on the 4x pyramid level
  PK_CONV_2X = 9,       // ... on the 2x level
  PK_OC1_UP = 10,       // output_conv1 with the fused resize
  PK_OC2_TAIL = 11,     // output_conv2 (32 channels) with the fused tail
  PK_COMM = 12,         // the all-gathers of a sharded forward
  PK_COUNT = 13
};

}  // namespace wm_host

struct wm_local_group {
  int world;
  pthread_barrier_t bar;
  std::vector<void*> recv;
};

struct wm_handle {
  wm_config cfg;
  int device = 0;
  std::string err;
  std::unordered_map<std::string, wm_host::Weight> w;
  std::map<std::string, std::vector<int64_t>> spec;
  bool finalized = false;
  wm_host::Comm comm;
  // workspace
  char* arena = nullptr;
  size_t arena_bytes = 0;
  bool arena_owned = true;   // false: caller-provided (wm_set_workspace)
  int plan_n = -1, plan_nt = -1, plan_H = -1, plan_W = -1;
  wm_host::TconvPack tconv[wm_host::HD_COUNT][2];   // per head and level: rebuilt by wm_reserve after a weight change
  bool tconv_valid = false;
  wm_host::Up1Comp up1comp[wm_host::HD_COUNT];      // per head, rebuilt with the token-conv packs
  wm_host::TapFold tapfold;                         // the heads' shared tap front, rebuilt with them
  std::vector<std::string> missing;  // names wm_finalize_weights filled with their init values
  // the weights and the workspace (with its shape-dependent device tables) as the forward reads them: bound by plan()
  wm_host::Model m;
  wm_host::Workspace ws;
  // Queues and events are created by wm_reserve (the heads') and by the communicator-init entries (the gather's): the forward only records
  // and waits.  The DPT heads are mutually independent: each runs on its own stream (forked/joined with events)
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
  static constexpr int NKIND = wm_host::PK_COUNT;
  std::vector<wm_host::EvPair> ev[NKIND];
  size_t ev_used[NKIND] = {};
};

namespace wm_host __attribute__((visibility("hidden"))) {   // (the attribute covers one namespace block, so it is repeated)

inline wm_status fail(wm_handle* h, wm_status st, const std::string& msg) {
  if (h) h->err = msg;
  return st;
}
#define HIPCHK(h, e)                                                                                   \
  do {                                                                                                 \
    hipError_t _e = (e);                                                                               \
    if (_e != hipSuccess)                                                                              \
      return fail(h, WM_ERR_HIP, std::string(hipGetErrorString(_e)) + " at " + __FILE__ + ":" + std::to_string(__LINE__)); \
  } while (0)

struct Dims {
  int n, nt, H, W, gh, gw, hw, Td, P, psi, D, heads, R, Md, Mv, Mx, kpad_patch, kpad_depth, world, chunk;
  int gh2, gw2;
};

// ---------------------------------------------------------------- profiling helpers
// (the one place where the forward still creates events, lazily and in profiling mode only: profiling serialises the heads anyway and is not
// the product path)
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

// ---------------------------------------------------------------- functions that cross files
// wm_weights.cpp (plan-time only: the forward reads the bound model)
const Weight* W(const wm_handle* h, const std::string& n);
// wm_compose.cpp
hipError_t launch_tconv(const TconvPack& t, int dt, const void* tokens16, float* out, int n, int gh, int gw, const void* zero16, hipStream_t s);
wm_status rebuild_weight_derived(wm_handle* h, const Dims& d);
// wm_plan.cpp
Dims make_dims(const wm_handle* h, int n, int nt, int H, int W);
// wm_comm.cpp
wm_status comm_allgather(wm_handle* h, const void* send, void* recv, size_t bytes, hipStream_t s);
// wm_backbone.cpp
wm_status gemm(Ctx& c, int dt, int epi, const void* A, int lda, const void* Wp, int ldw, void* C, int ldc, const float* bias,
               const float* gamma, int M, int N, int K, WmGemmArgs* extra = nullptr, int prof_kind = -1, bool* ln_fused = nullptr);
wm_status layernorm(Ctx& c, const WmLnArgs& a);
wm_status backbone_block(Ctx& c, const BlockW& w, float* X, int M, int seq_len, int heads, float eps,
                         bool rope, int tokens_per_view, int patch_start, bool is_global, float* tap_half = nullptr,
                         bool ln1_done = false, const Norm* next_norm1 = nullptr, bool* ln1_ready = nullptr);
// wm_heads.cpp
wm_status linear32(Ctx& c, const float* X, int ldx, const Lin32& w, float* Y, int ldy, int M, int pre, int post,
                   const float* gamma = nullptr, int accumulate = 0);
wm_status camera_head(Ctx& c, float* out_params);
wm_status tap_front_one(Ctx& c, const float* tap, void* xhat, const void* w16, const float* bias, const float* pos, int nh, int oc, int out16,
                        void* const* dst, int n, int hw, int P, int psi, int D2);
wm_status tap_front(Ctx& c);
wm_status dpt_head(Ctx& c, int id, int F_, int out_dim, int act, float* out_attr, float* out_conf,
                   const float* img, const wm_outputs* out, int first_view, int slot, bool front_done = false);

}  // namespace wm_host
