// Operator-level entries of the C ABI (include/wm_hip.h: wm_op_*), for tests and tools: each checks its pointers, fills one launcher's args
// struct, launches on the caller's stream and maps the hipError_t.  wm_op_tconv and wm_op_dpt_tap_front, at the end, run the forward's own
// building blocks through the orchestrator's internal header (wm_model.h).
#include <hip/hip_runtime.h>

#include <cstring>

#include "wm_api.h"
#include "wm_model.h"

extern "C" wm_status wm_op_gemm(int dtype, int epi, const void* A, const void* Wp, void* C, const float* bias, const float* gamma,
                                int M, int N, int K, void* stream) {
  WmGemmArgs a;
  memset(&a, 0, sizeof(a));
  a.A = A; a.W = Wp; a.C = C; a.bias = bias; a.gamma = gamma; a.M = M; a.N = N; a.K = K; a.lda = K; a.ldw = K; a.ldc = N;
  const int ldpad = wm_tune(WM_TUNE_OP_LDPAD, 0);   // wm_op_gemm only: operand row pitch K + ldpad (elements)
  if (ldpad > 0) a.lda = a.ldw = K + ldpad;
  a.dtype = dtype; a.epi = epi;
  return wm_launch_gemm(a, (hipStream_t)stream) == hipSuccess ? WM_OK : WM_ERR_HIP;
}
extern "C" wm_status wm_op_gemm_resid_ln(int dtype, const void* A, const void* Wp, float* X, const float* bias, const float* gamma, const float* ln_w,
                                         const float* ln_b, float ln_eps, void* ln_out, float* stats, int* sync, int M, int N, int K, int* fused_out,
                                         void* stream) {
  WmGemmArgs a;
  memset(&a, 0, sizeof(a));
  a.A = A; a.W = Wp; a.C = X; a.bias = bias; a.gamma = gamma; a.M = M; a.N = N; a.K = K; a.lda = K; a.ldw = K; a.ldc = N;
  a.dtype = dtype; a.epi = WM_EPI_RESID;
  a.ln_out = ln_out; a.ln_ld = N; a.ln_w = ln_w; a.ln_b = ln_b; a.ln_eps = ln_eps; a.ln_stats = stats; a.ln_sync = sync;
  a.ln_fallback = sync + ((size_t)M / 16 + 2) * 2;
  const bool fuse = wm_gemm_fuses_ln(a);
  if (fused_out) *fused_out = fuse ? 1 : 0;
  if (!fuse) a.ln_out = nullptr;
  if (wm_launch_gemm(a, (hipStream_t)stream) != hipSuccess) return WM_ERR_HIP;
  if (fuse && wm_launch_gemm_ln_fallback(a, (hipStream_t)stream) != hipSuccess) return WM_ERR_HIP;
  return WM_OK;
}
extern "C" wm_status wm_op_gemm_qkv(int dtype, const void* A, const void* Wp, const float* bias, void* q, void* k, void* v,
                                    const float* qn_w, const float* qn_b, const float* kn_w, const float* kn_b, const float* rope_cos,
                                    const float* rope_sin, int M, int H, int K, int tokens_per_view, int patch_start, int grid_w,
                                    float q_scale, void* stream) {
  WmGemmArgs a;
  memset(&a, 0, sizeof(a));
  a.A = A; a.W = Wp; a.bias = bias; a.M = M; a.N = 3 * H * 64; a.K = K; a.lda = K; a.ldw = K; a.dtype = dtype; a.epi = WM_EPI_QKV;
  a.qkv.q = q; a.qkv.k = k; a.qkv.v = v; a.qkv.qn_w = qn_w; a.qkv.qn_b = qn_b; a.qkv.kn_w = kn_w; a.qkv.kn_b = kn_b;
  a.qkv.rope_cos = rope_cos; a.qkv.rope_sin = rope_sin; a.qkv.M = M; a.qkv.H = H; a.qkv.head_stride = M;
  a.qkv.tokens_per_view = tokens_per_view; a.qkv.patch_start = patch_start; a.qkv.grid_w = grid_w; a.qkv.q_scale = q_scale; a.qkv.dtype = dtype;
  return wm_launch_gemm(a, (hipStream_t)stream) == hipSuccess ? WM_OK : WM_ERR_HIP;
}
// what the three attention entries share: the tensors, the sizes and the strides of a chunked K / V
static WmAttnArgs attn_args(int dtype, const void* Q, const void* K, const void* V, void* O, int H, int q_rows, int seq_len, int kv_chunks,
                            int kv_rows_per_chunk) {
  WmAttnArgs a;
  memset(&a, 0, sizeof(a));
  a.Q = Q; a.K = K; a.V = V; a.O = O; a.H = H; a.q_rows = q_rows; a.seq_len = seq_len; a.q_head_stride = q_rows;
  a.kv_chunks = kv_chunks; a.dtype = dtype;
  if (kv_chunks > 1) {
    a.kv_head_stride = kv_rows_per_chunk; a.kv_rows_per_chunk = kv_rows_per_chunk; a.kv_chunk_stride = (long long)H * kv_rows_per_chunk * 64;
  } else {
    a.kv_head_stride = q_rows;
  }
  return a;
}
extern "C" wm_status wm_op_attention(int dtype, const void* Q, const void* K, const void* V, void* O, int H, int q_rows, int seq_len,
                                     int kv_chunks, int kv_rows_per_chunk, void* stream) {
  const WmAttnArgs a = attn_args(dtype, Q, K, V, O, H, q_rows, seq_len, kv_chunks, kv_rows_per_chunk);
  return wm_launch_attention(a, (hipStream_t)stream) == hipSuccess ? WM_OK : WM_ERR_HIP;
}
extern "C" wm_status wm_op_attention_split(int dtype, const void* Q, const void* K, const void* V, void* O, int H, int q_rows, int seq_len,
                                           int kv_chunks, int kv_rows_per_chunk, int kv_splits, float* part_o, float* part_ml, void* stream) {
  WmAttnArgs a = attn_args(dtype, Q, K, V, O, H, q_rows, seq_len, kv_chunks, kv_rows_per_chunk);
  a.kv_splits = kv_splits; a.max_splits = WM_ATTN_MAX_SPLITS; a.part_o = part_o; a.part_ml = part_ml;
  return wm_launch_attention(a, (hipStream_t)stream) == hipSuccess ? WM_OK : WM_ERR_HIP;
}
extern "C" wm_status wm_op_attention_ex(int dtype, const void* Q, const void* K, const void* V, void* O, int H, int q_rows, int seq_len,
                                        int kv_chunks, int kv_rows_per_chunk, int kv_splits, float* part_o, float* part_ml, int* unit_flags,
                                        void* stream) {
  WmAttnArgs a = attn_args(dtype, Q, K, V, O, H, q_rows, seq_len, kv_chunks, kv_rows_per_chunk);
  a.kv_splits = kv_splits; a.max_splits = WM_ATTN_MAX_SPLITS; a.part_o = part_o; a.part_ml = part_ml;
  a.unit_flags = unit_flags;
  // the second half of the caller's flag buffer holds the sticky hints (wm_op_attention_flag_count counts both halves): a caller that
  // reuses one zero-initialised buffer across calls gets the forward's behaviour, one that clears it per call the hint-free one
  if (unit_flags) {
    const size_t nb = wm_attention_max_blocks(q_rows, seq_len, H);
    a.unit_hint = unit_flags + nb;
    a.unit_stat = unit_flags + 2 * nb;
    // the forward's host policy (backbone_block) for ONE buffer at a time, when the tuning key attn_op_policy is 1 (tools/bench_attn_v4.py)
    const bool policy = wm_tune(WM_TUNE_ATTN_OP_POLICY, 0) == 1;
    static int* mirror = nullptr;
    static const int* key = nullptr;
    static int seen = 0, ttl = 0;
    if (!mirror && hipHostMalloc((void**)&mirror, 4, hipHostMallocDefault) != hipSuccess) return WM_ERR_HIP;
    if (key != unit_flags) { key = unit_flags; seen = 0; ttl = 0; *mirror = 0; }
    const int cur = *mirror, delta = cur - seen;
    seen = cur;
    const long units = (long)((seq_len + 511) / 512) * (q_rows / (seq_len > 0 ? seq_len : 1)) * H;
    if (delta < 0) ttl = 0;                                   // the caller cleared its buffer
    else if (delta > 0 && (long)delta * 4 >= units) ttl = WM_ATTN_HINT_TTL;
    const bool general_only = policy && ttl > 0;
    if (general_only) --ttl;
    int* stat = a.unit_stat;
    if (general_only) { a.unit_flags = nullptr; a.unit_hint = nullptr; a.unit_stat = nullptr; }
    if (wm_launch_attention(a, (hipStream_t)stream) != hipSuccess) return WM_ERR_HIP;
    return hipMemcpyAsync(mirror, stat, 4, hipMemcpyDeviceToHost, (hipStream_t)stream) == hipSuccess ? WM_OK : WM_ERR_HIP;
  }
  return wm_launch_attention(a, (hipStream_t)stream) == hipSuccess ? WM_OK : WM_ERR_HIP;
}
// ints of the caller's buffer: [flags | sticky hints | 1 fallback counter (+ pad)]
extern "C" size_t wm_op_attention_flag_count(int q_rows, int seq_len, int H) { return 2 * wm_attention_max_blocks(q_rows, seq_len, H) + 4; }
// resize (align_corners bilinear + position tables) to 16 bits, then the 32-channel 3x3 conv on it: the unfused form of
// wm_op_conv3x3_up for Cout == 32.  up16: Hi * Wi * N * Cin 16-bit elements + 16 B of scratch (zeroed here).
extern "C" wm_status wm_op_up_conv_n32(int dtype, const float* x, const void* w16, const float* bias, float* y, int N, int Hs, int Ws, int Hi,
                                       int Wi, int Cin, const float* addx, const float* addy, int relu_out, void* up16, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (Cin % 64 || !up16) return WM_ERR_INVALID;
  const size_t n16 = (size_t)N * Hi * Wi * Cin;
  uint16_t* zero = (uint16_t*)up16 + ((n16 + 7) & ~(size_t)7);
  if (hipMemsetAsync(zero, 0, 16, s) != hipSuccess) return WM_ERR_HIP;
  if (wm_launch_bilinear16(x, up16, N, Hs, Ws, Hi, Wi, Cin, addx, addy, dtype, s) != hipSuccess) return WM_ERR_HIP;
  WmConvN32Args a;
  memset(&a, 0, sizeof(a));
  a.x = (const uint16_t*)up16; a.w = (const uint16_t*)w16; a.bias = bias; a.y = y; a.zero = zero;
  a.N = N; a.H = Hi; a.W = Wi; a.Cin = Cin; a.relu_out = relu_out; a.dtype = dtype;
  return wm_launch_conv3x3_n32_in16(a, s) == hipSuccess ? WM_OK : WM_ERR_HIP;
}
// splat assembly of prepare_splats (rasterization.py:389-498) as an operator: the launch the forward makes behind the gs head, for the
// parity tests (tests/test_gpu_ops_tails.py) and tools/micro/splat_hazard_repro.cpp
extern "C" wm_status wm_op_gs_splat(const float* gp, const float* img, const float* depth, const float* cam, float* means, float* quats,
                                    float* scales, float* opac, float* sh, float* wts, int N, int H, int W, void* stream) {
  return wm_launch_gs_splat(gp, img, depth, cam, means, quats, scales, opac, sh, wts, N, H, W, (hipStream_t)stream) == hipSuccess ? WM_OK : WM_ERR_HIP;
}
extern "C" wm_status wm_op_layernorm(const float* x, void* y, const float* w, const float* b, int rows, int D, float eps, int out_f32,
                                     int dtype, void* stream) {
  WmLnArgs a;
  memset(&a, 0, sizeof(a));
  a.x = x; a.y = y; a.w = w; a.b = b; a.D = D; a.ld_in = D; a.ld_out = D; a.eps = eps; a.groups = 1; a.rows_per_group = rows;
  a.out_f32 = out_f32; a.dtype = dtype;
  return wm_launch_layernorm(a, (hipStream_t)stream) == hipSuccess ? WM_OK : WM_ERR_HIP;
}
extern "C" wm_status wm_op_qkv_post(int dtype, const float* qkv, void* q, void* k, void* v, const float* qn_w, const float* qn_b,
                                    const float* kn_w, const float* kn_b, const float* rope_cos, const float* rope_sin, int M, int H,
                                    int tokens_per_view, int patch_start, int grid_w, float q_scale, void* stream) {
  WmQkvArgs a;
  memset(&a, 0, sizeof(a));
  a.qkv = qkv; a.q = q; a.k = k; a.v = v; a.qn_w = qn_w; a.qn_b = qn_b; a.kn_w = kn_w; a.kn_b = kn_b; a.rope_cos = rope_cos; a.rope_sin = rope_sin;
  a.M = M; a.H = H; a.head_stride = M; a.tokens_per_view = tokens_per_view; a.patch_start = patch_start; a.grid_w = grid_w; a.q_scale = q_scale;
  a.dtype = dtype;
  return wm_launch_qkv_post(a, (hipStream_t)stream) == hipSuccess ? WM_OK : WM_ERR_HIP;
}
extern "C" wm_status wm_op_conv(int dtype, const float* x, const void* w16, const float* bias, const float* resid, const float* resid2,
                                float* y, int N, int Hi, int Wi, int Cin, int Cout, int ksize, int stride, int pad, int relu_in,
                                int resid_relu, void* stream) {
  WmConvArgs a;
  memset(&a, 0, sizeof(a));
  a.x = x; a.w = w16; a.bias = bias; a.resid = resid; a.resid2 = resid2; a.y = y; a.N = N; a.Hi = Hi; a.Wi = Wi; a.Cin = Cin; a.Cout = Cout;
  a.ksize = ksize; a.stride = stride; a.pad = pad; a.Ho = (Hi + 2 * pad - ksize) / stride + 1; a.Wo = (Wi + 2 * pad - ksize) / stride + 1;
  a.relu_in = relu_in; a.resid_relu = resid_relu; a.dtype = dtype;
  return wm_launch_conv(a, (hipStream_t)stream) == hipSuccess ? WM_OK : WM_ERR_HIP;
}
// wm_op_conv with the 16-bit tensor forms of the register-staged 3x3 kernel: x is 16-bit NHWC when in16 (relu_in must be 0), y is 16-bit NHWC
// when out16 (refused with WM_ERR_INVALID when the launch would take a kernel without that form: wm_conv3x3_out16_ok)
extern "C" wm_status wm_op_conv_ex(int dtype, const void* x, int in16, const void* w16, const float* bias, const float* resid, const float* resid2,
                                   void* y, int out16, int N, int Hi, int Wi, int Cin, int Cout, int relu_in, int resid_relu, int relu_out, void* stream) {
  WmConvArgs a;
  memset(&a, 0, sizeof(a));
  a.x = (const float*)x; a.w = w16; a.bias = bias; a.resid = resid; a.resid2 = resid2; a.y = (float*)y; a.N = N; a.Hi = Hi; a.Wi = Wi; a.Cin = Cin; a.Cout = Cout;
  a.ksize = 3; a.stride = 1; a.pad = 1; a.Ho = Hi; a.Wo = Wi; a.relu_in = relu_in; a.resid_relu = resid_relu; a.relu_out = relu_out; a.dtype = dtype;
  a.in16 = in16; a.out16 = out16;
  if ((in16 || out16) && !wm_conv3x3_out16_ok(a)) return WM_ERR_INVALID;
  return wm_launch_conv(a, (hipStream_t)stream) == hipSuccess ? WM_OK : WM_ERR_HIP;
}
// Conv2d(C, Co, 3, padding=1)(F.interpolate(x, (Ho, Wo), bilinear, align_corners=True)) in the tap form of upconv.hip on a 16-bit (f16) NHWC x:
// wt16: scratch of 9 Co C 16-bit elements (the tap-major weight copy), y16: scratch of N Hi Wi 9 Co 16-bit elements
extern "C" wm_status wm_op_upconv3x3_tap(int dtype, const void* x16, const void* w16, const float* bias, float* out, int N, int Hi, int Wi, int Ho,
                                         int Wo, int C, int Co, void* wt16, void* y16, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (dtype != WM_DT_F16 || !x16 || !w16 || !out || !wt16 || !y16 || C % 64) return WM_ERR_INVALID;
  if (wm_launch_repack_tap_major(w16, wt16, Co, C, s) != hipSuccess) return WM_ERR_HIP;
  WmGemmArgs g;
  memset(&g, 0, sizeof(g));
  g.A = x16; g.W = wt16; g.C = y16; g.M = N * Hi * Wi; g.N = 9 * Co; g.K = C; g.lda = C; g.ldw = C; g.ldc = 9 * Co; g.dtype = dtype; g.epi = WM_EPI_T16;
  if (wm_launch_gemm(g, s) != hipSuccess) return WM_ERR_HIP;
  return wm_launch_upconv_gather(y16, bias, out, N, Hi, Wi, Ho, Wo, Co, s) == hipSuccess ? WM_OK : WM_ERR_HIP;
}
extern "C" wm_status wm_op_upconv_gather(const void* y16, const float* bias, float* out, int N, int Hi, int Wi, int Ho, int Wo, int Co, void* stream) {
  return wm_launch_upconv_gather(y16, bias, out, N, Hi, Wi, Ho, Wo, Co, (hipStream_t)stream) == hipSuccess ? WM_OK : WM_ERR_HIP;
}
extern "C" wm_status wm_op_conv3x3_gemm16(int dtype, const void* x16, const void* w16, const float* bias, const float* resid, int resid_relu,
                                          const float* resid2, void* y, int out16, int relu_out, int N, int H, int W, int Cin, int Cout,
                                          const void* zero16, void* stream) {
  if (N <= 0 || H <= 0 || W <= 0 || Cin % 64 || (Cout & 7) || !zero16 || !x16 || !w16 || !y) return WM_ERR_INVALID;
  WmGemmArgs g;
  memset(&g, 0, sizeof(g));
  g.A = x16; g.W = w16; g.C = y; g.bias = bias; g.M = N * H * W; g.N = Cout; g.K = 9 * Cin; g.lda = Cin; g.ldw = 9 * Cin; g.ldc = Cout;
  g.dtype = dtype; g.epi = WM_EPI_CONV; g.cv_h = H; g.cv_w = W; g.cv_cin = Cin; g.cv_zero = zero16;
  g.cv_resid = resid; g.cv_resid2 = resid2; g.cv_resid_relu = resid_relu; g.out16 = out16; g.relu = relu_out;
  return wm_launch_gemm(g, (hipStream_t)stream) == hipSuccess ? WM_OK : WM_ERR_HIP;
}
extern "C" wm_status wm_op_conv3x3_up(int dtype, const float* x, const void* w16, const float* bias, float* y, int N, int Hs, int Ws, int Hi, int Wi,
                                      int Cin, int Cout, const float* addx, const float* addy, void* stream) {
  WmConvArgs a;
  memset(&a, 0, sizeof(a));
  a.x = x; a.w = w16; a.bias = bias; a.y = y; a.N = N; a.Hi = Hi; a.Wi = Wi; a.Cin = Cin; a.Cout = Cout; a.ksize = 3; a.stride = 1; a.pad = 1;
  a.Ho = Hi; a.Wo = Wi; a.dtype = dtype; a.up_hs = Hs; a.up_ws = Ws; a.up_addx = addx; a.up_addy = addy;
  return wm_launch_conv(a, (hipStream_t)stream) == hipSuccess ? WM_OK : WM_ERR_HIP;
}
extern "C" wm_status wm_op_bilinear(const float* in, float* out, int N, int Hi, int Wi, int Ho, int Wo, int C, void* stream) {
  return wm_launch_bilinear(in, out, N, Hi, Wi, Ho, Wo, C, nullptr, nullptr, (hipStream_t)stream) == hipSuccess ? WM_OK : WM_ERR_HIP;
}
extern "C" wm_status wm_op_linear_f32(const float* X, const float* Wp, const float* b, float* Y, int M, int N, int K, int ldx, int pre_act,
                                      int post_act, void* stream) {
  return wm_launch_linear_f32(X, Wp, b, Y, M, N, K, ldx, N, pre_act, post_act, nullptr, 0, (hipStream_t)stream) == hipSuccess ? WM_OK : WM_ERR_HIP;
}

// ---- operator-level entry points of the token front end and the camera head (tests/test_gpu_ops_frontend.py): args struct, launcher, status
extern "C" wm_status wm_op_im2col(int dtype, const float* img, void* out, int N, int C, int H, int W, int ps, int Kpad, int normalize,
                                  void* stream) {
  if (!img || !out || N < 0 || C <= 0 || H <= 0 || W <= 0 || ps <= 0 || Kpad < C * ps * ps || (normalize && C != 3)) return WM_ERR_INVALID;
  return wm_status_of(wm_launch_im2col(img, out, N, C, H, W, ps, Kpad, normalize, dtype, (hipStream_t)stream));
}
extern "C" wm_status wm_op_im2col7(int dtype, const float* img, void* out, int N, int H, int W, int Kpad, void* stream) {
  if (!img || !out || N < 0 || H <= 0 || W <= 0 || Kpad < 147) return WM_ERR_INVALID;
  return wm_status_of(wm_launch_im2col7(img, out, N, H, W, Kpad, dtype, (hipStream_t)stream));
}
extern "C" wm_status wm_op_dino_tokens(const float* patch, const float* cls, const float* reg, const float* pos, float* X, int N, int hw,
                                       int R, int D, void* stream) {
  if (!cls || !pos || !X || (R > 0 && !reg) || N <= 0 || hw < 0 || R < 0 || D <= 0) return WM_ERR_INVALID;
  return wm_status_of(wm_launch_dino_tokens(patch, cls, reg, pos, X, N, hw, R, D, (hipStream_t)stream));
}
extern "C" wm_status wm_op_vgt_special(float* X, const float* cam_tok, const float* reg_tok, const float* pose_tok, const float* ray_tok,
                                       int N, int P, int R, int D, int cond, int first_view_global, void* stream) {
  if (!X || !cam_tok || (R > 0 && !reg_tok) || N <= 0 || R < 0 || D <= 0 || P < 1 + R + (cond ? 2 : 0)) return WM_ERR_INVALID;
  return wm_status_of(wm_launch_vgt_special(X, cam_tok, reg_tok, pose_tok, ray_tok, N, P, R, D, cond, first_view_global, (hipStream_t)stream));
}
extern "C" wm_status wm_op_gemm_rowmap(int dtype, const void* A, const void* Wp, void* C, const float* bias, const float* add, int M, int N,
                                       int K, int ldc, int rows_per_group, int out_group, int out_off, int accumulate, int out16, int relu,
                                       void* stream) {
  if (rows_per_group <= 0 || out_group < 0 || out_off < 0 || ldc < N || (out16 && accumulate)) return WM_ERR_INVALID;
  WmGemmArgs a;
  memset(&a, 0, sizeof(a));
  a.A = A; a.W = Wp; a.C = C; a.bias = bias; a.add = add; a.M = M; a.N = N; a.K = K; a.lda = K; a.ldw = K; a.ldc = ldc;
  a.dtype = dtype; a.epi = WM_EPI_ROWMAP_ADD;
  a.rows_per_group = rows_per_group; a.out_group = out_group; a.out_off = out_off; a.accumulate = accumulate; a.out16 = out16; a.relu = relu;
  return wm_status_of(wm_launch_gemm(a, (hipStream_t)stream));
}
extern "C" wm_status wm_op_gemm_convt(int dtype, const void* A, const void* Wp, float* C, const float* bias, int M, int N, int K, int ct_k,
                                      int ct_cout, int ct_gh, int ct_gw, void* stream) {
  if (!bias || ct_k <= 0 || ct_cout <= 0 || ct_gh <= 0 || ct_gw <= 0 || N != ct_k * ct_k * ct_cout || M % (ct_gh * ct_gw)) return WM_ERR_INVALID;
  WmGemmArgs a;
  memset(&a, 0, sizeof(a));
  a.A = A; a.W = Wp; a.C = C; a.bias = bias; a.M = M; a.N = N; a.K = K; a.lda = K; a.ldw = K; a.ldc = 0;
  a.dtype = dtype; a.epi = WM_EPI_CONVT;
  a.ct_k = ct_k; a.ct_cout = ct_cout; a.ct_gh = ct_gh; a.ct_gw = ct_gw;
  return wm_status_of(wm_launch_gemm(a, (hipStream_t)stream));
}
extern "C" wm_status wm_op_layernorm_rows(const float* x, void* y, const float* w, const float* b, int D, int ld_in, int ld_out, float eps,
                                          int groups, int rows_per_group, int in_group, int in_off, int out_group, int out_off, int out_f32,
                                          int dtype, void* stream) {
  if (!x || !y || D <= 0 || ld_in < D || ld_out < D || groups < 0 || rows_per_group <= 0 || in_group < 0 || in_off < 0 || out_group < 0 || out_off < 0)
    return WM_ERR_INVALID;
  WmLnArgs a;
  memset(&a, 0, sizeof(a));
  a.x = x; a.y = y; a.w = w; a.b = b; a.D = D; a.ld_in = ld_in; a.ld_out = ld_out; a.eps = eps;
  a.groups = groups; a.rows_per_group = rows_per_group; a.in_group = in_group; a.in_off = in_off; a.out_group = out_group; a.out_off = out_off;
  a.out_f32 = out_f32; a.dtype = dtype;
  return wm_status_of(wm_launch_layernorm(a, (hipStream_t)stream));
}
extern "C" wm_status wm_op_bilinear_add(const float* in, float* out, int N, int Hi, int Wi, int Ho, int Wo, int C, const float* addx,
                                        const float* addy, void* stream) {
  if (!in || !out || N < 0 || Hi <= 0 || Wi <= 0 || Ho <= 0 || Wo <= 0 || C <= 0 || (addx != nullptr) != (addy != nullptr)) return WM_ERR_INVALID;
  return wm_status_of(wm_launch_bilinear(in, out, N, Hi, Wi, Ho, Wo, C, addx, addy, (hipStream_t)stream));
}
extern "C" wm_status wm_op_bilinear16(int dtype, const float* in, void* out16, int N, int Hi, int Wi, int Ho, int Wo, int C, const float* addx,
                                      const float* addy, void* stream) {
  // C % 8: the position tables are read as whole float4s on either side of C / 2
  if (!in || !out16 || N < 0 || Hi <= 0 || Wi <= 0 || Ho <= 0 || Wo <= 0 || C <= 0 || (addx != nullptr) != (addy != nullptr) || (addx && C % 8))
    return WM_ERR_INVALID;
  return wm_status_of(wm_launch_bilinear16(in, out16, N, Hi, Wi, Ho, Wo, C, addx, addy, dtype, (hipStream_t)stream));
}
extern "C" wm_status wm_op_copy2d(const float* src, float* dst, int rows, int cols, int ld_src, int ld_dst, void* stream) {
  if (!src || !dst || rows < 0 || cols <= 0 || ld_src < cols || ld_dst < cols) return WM_ERR_INVALID;
  return wm_status_of(wm_launch_copy2d(src, dst, rows, cols, ld_src, ld_dst, (hipStream_t)stream));
}
extern "C" wm_status wm_op_small_attention(const float* qkv, float* out, int S, int heads, int hd, void* stream) {
  if (!qkv || !out || S < 0 || heads <= 0 || hd <= 0) return WM_ERR_INVALID;
  return wm_status_of(wm_launch_small_attention(qkv, out, S, heads, hd, (hipStream_t)stream));
}
extern "C" wm_status wm_op_adaln(const float* tok, const float* mod, float* h, int S, int D, float eps, void* stream) {
  if (!tok || !mod || !h || S < 0 || D <= 0) return WM_ERR_INVALID;
  return wm_status_of(wm_launch_adaln(tok, mod, h, S, D, eps, (hipStream_t)stream));
}
extern "C" wm_status wm_op_cam_update(float* pred, const float* delta, float* out, int S, int first, void* stream) {
  if (!pred || !delta || !out || S < 0) return WM_ERR_INVALID;
  return wm_status_of(wm_launch_cam_update(pred, delta, out, S, first, (hipStream_t)stream));
}
extern "C" wm_status wm_op_cam_matrices(const float* params, float* poses, float* intrs, int S, int H, int W, void* stream) {
  if (!params || !poses || !intrs || S < 0) return WM_ERR_INVALID;
  return wm_status_of(wm_launch_cam_matrices(params, poses, intrs, S, H, W, (hipStream_t)stream));
}
extern "C" wm_status wm_op_linear_f32_ex(const float* X, const float* Wp, const float* b, float* Y, int M, int N, int K, int ldx, int ldy,
                                         int pre_act, int post_act, const float* gamma, int accumulate, void* stream) {
  if (!X || !Wp || !Y || K <= 0 || ldx < K || ldy < N) return WM_ERR_INVALID;
  return wm_status_of(wm_launch_linear_f32(X, Wp, b, Y, M, N, K, ldx, ldy, pre_act, post_act, gamma, accumulate, (hipStream_t)stream));
}
extern "C" wm_status wm_op_dpt_tail(const float* y32, const float* w, const float* b, float* attr, float* conf, size_t npix, int C, int act,
                                    void* stream) {
  if (!y32 || !w || !b || !attr || !conf || act < WM_ACT_INV_LOG || act > WM_ACT_NORM) return WM_ERR_INVALID;
  return wm_status_of(wm_launch_dpt_tail(y32, w, b, attr, conf, npix, C, act, (hipStream_t)stream));   // the launcher refuses C outside 2..4
}
// wm_op_up_conv_n32 with the head's tail in the conv's epilogue: the launch pair dpt_head makes for output_conv2 when dpt_features / 2 is a
// multiple of 64 (the 32-channel tensor is never stored)
extern "C" wm_status wm_op_up_conv_n32_tail(int dtype, const float* x, const void* w16, const float* bias, int N, int Hs, int Ws, int Hi, int Wi,
                                            int Cin, const float* addx, const float* addy, const float* tail_w, const float* tail_b, int tail_C,
                                            int tail_act, float* attr, float* conf, void* up16, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if ((dtype != WM_DT_BF16 && dtype != WM_DT_F16) || !x || !w16 || !up16 || !tail_w || !tail_b || !attr || !conf || N < 0 || Hs <= 0 || Ws <= 0 || Hi <= 0 || Wi <= 0 || Cin <= 0 || Cin % 64 || Cin > 128 ||
      (addx != nullptr) != (addy != nullptr) || tail_act < WM_ACT_INV_LOG || tail_act > WM_ACT_NORM || tail_C < 2 || tail_C > 4)
    return WM_ERR_INVALID;
  const size_t n16 = (size_t)N * Hi * Wi * Cin;
  uint16_t* zero = (uint16_t*)up16 + ((n16 + 7) & ~(size_t)7);
  if (hipMemsetAsync(zero, 0, 16, s) != hipSuccess) return WM_ERR_HIP;
  const wm_status st = wm_status_of(wm_launch_bilinear16(x, up16, N, Hs, Ws, Hi, Wi, Cin, addx, addy, dtype, s));
  if (st != WM_OK) return st;
  WmConvN32Args a;
  memset(&a, 0, sizeof(a));
  a.x = (const uint16_t*)up16; a.w = (const uint16_t*)w16; a.bias = bias; a.zero = zero;
  a.N = N; a.H = Hi; a.W = Wi; a.Cin = Cin; a.relu_out = 0; a.dtype = dtype;
  a.tail_w = tail_w; a.tail_b = tail_b; a.tail_C = tail_C; a.tail_act = tail_act; a.tail_attr = attr; a.tail_conf = conf;
  return wm_status_of(wm_launch_conv3x3_n32_in16(a, s));
}

// ====================================================================================== the forward's own building blocks
using namespace wm_host;

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
