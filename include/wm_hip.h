/* libwm_hip.so — C ABI of the MI355X-native WorldMirror forward pass.
 *
 * The reference (zubair-irshad/HunyuanWorld-Mirror) has no FFI/operator layer on this path: its
 * boundary is the Python class WorldMirror (src/models/models/worldmirror.py:16) whose forward()
 * (:120-152) is pure torch.nn.  This header is the boundary a maintainer binds instead (ctypes stub
 * in INTEGRATION.md); each entry cites the reference call it replaces.  Plain pointers and sizes
 * only; device pointers are HIP device memory owned by the caller (torch-ROCm tensors in practice).
 *
 * Threading: one handle per (process, device); calls on a handle are serialised by the caller and
 * are stream-ordered on the hipStream_t passed in (hipStream_t is passed as void*).
 */
#ifndef WM_HIP_H
#define WM_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct wm_handle wm_handle;

typedef enum { WM_OK = 0, WM_ERR_INVALID = 1, WM_ERR_HIP = 2, WM_ERR_STATE = 3, WM_ERR_COMM = 4 } wm_status;
typedef enum { WM_DT_BF16 = 0, WM_DT_F16 = 1 } wm_dtype;

/* Architecture: reference ctor kwargs (worldmirror.py:17-34) + the sub-module defaults they imply
 * (visual_transformer.py:48-70, vision_transformer.py:364-375, camera_head.py:16-27,
 * dense_head.py:34-46). */
typedef struct {
  int32_t img_size, patch_size, embed_dim, gs_dim;
  int32_t enable_cond, enable_cam, enable_pts, enable_depth, enable_norm, enable_gs;
  int32_t depth, num_heads, mlp_ratio, num_register_tokens;
  int32_t intermediate_idxs[4];
  float rope_freq;
  int32_t dino_depth, dino_heads;
  int32_t cam_trunk_depth, cam_heads, cam_steps;
  int32_t dpt_features;
  int32_t dpt_out_channels[4];
  int32_t backbone_dtype; /* wm_dtype of GEMM/attention operands inside the backbone (reference GPU recipe: bf16) */
  int32_t head_dtype;     /* wm_dtype of DPT conv operands (fp32 accumulate/activations; default f16)          */
} wm_config;

/* Outputs of WorldMirror.forward (worldmirror.py:157-216), caller-allocated f32 device buffers for
 * the LOCAL views; any pointer may be NULL to skip that output (a NULL dense output skips its head). */
typedef struct {
  float* camera_params; /* [N_total][9]  (camera head attends across all views) */
  float* camera_poses;  /* [N_total][4][4] c2w */
  float* camera_intrs;  /* [N_total][3][3] */
  float* depth;         /* [N][H][W][1] */
  float* depth_conf;    /* [N][H][W]    */
  float* pts3d;         /* [N][H][W][3] */
  float* pts3d_conf;    /* [N][H][W]    */
  float* normals;       /* [N][H][W][3] */
  float* normals_conf;  /* [N][H][W]    */
  float* gs_depth;      /* [N][H][W][1] */
  float* gs_depth_conf; /* [N][H][W]    */
  /* Gaussian splats before voxel pruning (rasterization.py:389-498), one per pixel of the local views */
  float* splat_means;     /* [N][H][W][3] */
  float* splat_quats;     /* [N][H][W][4] */
  float* splat_scales;    /* [N][H][W][3] */
  float* splat_opacities; /* [N][H][W]    */
  float* splat_sh;        /* [N][H][W][3] (sh degree 0) */
  float* splat_weights;   /* [N][H][W]    */
  float* taps[4];       /* optional: the 4 backbone taps [N][P][2*D] (visual_transformer.py:337-339) */
} wm_outputs;

/* ---- lifecycle (replaces WorldMirror.__init__ / from_pretrained / load_state_dict) ---- */
wm_status wm_create(const wm_config* cfg, int device, wm_handle** out);
void wm_destroy(wm_handle* h);
const char* wm_last_error(const wm_handle* h);
/* One reference state_dict tensor (fp32, host memory). Unknown names are ignored (strict=False). */
wm_status wm_set_weight(wm_handle* h, const char* name, const float* host, const int64_t* shape, int ndim);
/* Number of spec'd parameters still missing is written to *missing.  strict=False semantics of the reference's loader
 * (PyTorchModelHubMixin, src/models/models/worldmirror.py:13,16): a missing tensor keeps its init value where that
 * value is deterministic — LayerNorm 1 / 0, LayerScale gamma 1.0 in the DINOv2 encoder and 0.01 elsewhere
 * (visual_transformer.py:65,152-160; camera_head.py:24) — the rest (randomly initialised in the reference) is 0.
 * wm_missing_name(h, i), i < *missing, lists them (NULL past the end). */
wm_status wm_finalize_weights(wm_handle* h, int* missing);
const char* wm_missing_name(const wm_handle* h, int i);
/* Several handles on ONE device (one per stream / per in-process rank) can share one copy of the repacked weights:
 * dst (same wm_config, same device) refers to src's device tensors without copying; src must outlive dst and must not
 * be re-loaded while dst exists.  The nn.Module analogue is several callers sharing one model's parameters. */
wm_status wm_share_weights(wm_handle* dst, const wm_handle* src);
/* DINO pos-embed resample for a non-native grid is done inside the library (host, once per shape);
 * exported for tests: in [gs*gs][D] -> out [gh*gw][D], bicubic antialias (vision_transformer.py:175-207). */
void wm_host_resample_pos(const float* in, int gs, int D, int gh, int gw, float* out);

/* ---- forward (replaces WorldMirror.forward, worldmirror.py:120-152) ---- */
size_t wm_workspace_bytes(const wm_handle* h, int n_local, int n_total, int H, int W);
/* Workspace ownership ("no hidden allocation in wm_forward").  wm_forward / wm_forward_sharded never allocate,
 * synchronise or build tables: the workspace for the call's shape must have been prepared by wm_reserve, which sizes
 * (wm_workspace_bytes) and lays out the arena and uploads the shape- and weight-derived tables (RoPE, resampled
 * pos_embed of vision_transformer.py:175-207, the DPT UV tables of dense_head.py:253-263).  Call it again after a
 * shape change or after wm_set_weight / wm_finalize_weights; a forward without it returns WM_ERR_STATE.
 * The arena is the library's (hipMalloc inside wm_reserve, grown only when a shape needs more) unless the caller
 * provides device memory with wm_set_workspace (NULL returns ownership to the library): then wm_reserve fails with
 * WM_ERR_STATE instead of allocating when `bytes` < wm_workspace_bytes(...). */
wm_status wm_reserve(wm_handle* h, int n_local, int n_total, int H, int W);
wm_status wm_set_workspace(wm_handle* h, void* device_ptr, size_t bytes);
/* img [N][3][H][W] f32 in [0,1]; priors already normalised as extract_priors returns them
 * (worldmirror.py:218-251): pose7 [N][7], depth [N][H][W], ray4 [N][4]; any may be NULL.
 * cond_flags = [pose, depth, rays]. */
wm_status wm_forward(wm_handle* h, const float* img, int N, int H, int W, const float* pose7, const float* depth,
                     const float* ray4, const int32_t cond_flags[3], const wm_outputs* out, void* stream);
/* View-sharded forward: this rank owns views [first_view, first_view + n_local) of n_total; K/V of
 * every global-attention layer and the camera tokens are all-gathered through the handle's comm. */
wm_status wm_forward_sharded(wm_handle* h, const float* img, int n_local, int first_view, int n_total, int H, int W,
                             const float* pose7, const float* depth, const float* ray4, const int32_t cond_flags[3],
                             const wm_outputs* out, void* stream);

/* ---- communicator for the sharded path ---- */
#define WM_RCCL_ID_BYTES 128
wm_status wm_rccl_unique_id(uint8_t id[WM_RCCL_ID_BYTES]);
wm_status wm_comm_init_rccl(wm_handle* h, const uint8_t id[WM_RCCL_ID_BYTES], int rank, int world);
/* In-process group (ranks = host threads, one handle each, possibly sharing one GPU): used by tests. */
typedef struct wm_local_group wm_local_group;
wm_local_group* wm_local_group_create(int world);
void wm_local_group_destroy(wm_local_group* g);
wm_status wm_comm_init_local(wm_handle* h, wm_local_group* g, int rank);
/* All-gather over the handle's communicator (RCCL, or the in-process group), stream-ordered: recv = [world][bytes_per_rank].
 * For the ONE cross-view step behind the forward: the reference's prune_gs merges the splats of ALL views
 * (src/models/models/rasterization.py:301-387), so a sharded forward gathers the per-rank raw splats before the merge. */
wm_status wm_allgather(wm_handle* h, const void* send, void* recv, size_t bytes_per_rank, void* stream);

/* ---- timing hooks used by bench.py: HIP events on the launch stream around kernel classes ---- */
/* kind: 0 = global attention, 1 = frame+dino attention, 2 = GEMM (epilogues other than the three below), 3 = DPT conv,
 * 4 = whole forward, 5 = GEMM with the fused qkv epilogue, 6 = GEMM with the LayerScale+residual epilogue (proj, fc2),
 * 7 = GEMM with the GELU epilogue (fc1), 8 / 9 = DPT 3x3 convs F -> F on the 4x / 2x pyramid levels, 10 = output_conv1 with the
 * fused resize, 11 = output_conv2 (32 channels) with the fused tail; 3 then holds the remaining convs; 12 = the all-gathers of a
 * sharded forward (K|V per global layer + the camera tokens), timed on the queue they run on: with the gather on the compute
 * queue (the default) that is the time the collective is exposed */
wm_status wm_profile_enable(wm_handle* h, int on);
wm_status wm_profile_read(wm_handle* h, int kind, double* total_ms, int64_t* launches);

/* ---- operator-level entry points (device pointers) used by the parity tests ---- */
wm_status wm_op_gemm(int dtype, int epi, const void* A, const void* W, void* C, const float* bias, const float* gamma,
                     int M, int N, int K, void* stream);
/* QKV projection with the q/k-norm + 2-D RoPE + head-major relayout epilogue (attention.py:50-56): A [M][K] 16-bit,
 * W [3*H*64][K] 16-bit -> q,k,v 16-bit [H][M][64] */
wm_status wm_op_gemm_qkv(int dtype, const void* A, const void* W, const float* bias, void* q, void* k, void* v, const float* qn_w,
                         const float* qn_b, const float* kn_w, const float* kn_b, const float* rope_cos, const float* rope_sin, int M,
                         int H, int K, int tokens_per_view, int patch_start, int grid_w, float q_scale, void* stream);
/* X[M][1024] += gamma * (A W^T + bias) with the FOLLOWING LayerNorm fused into the epilogue (round 4: block.py:44,61 behind :90-92;
   mlp.py:29-35 / attention.py:67): ln_out[M][1024] (16-bit, the operand type) = LayerNorm(X_new) * ln_w + ln_b.  stats: M * 8 floats of
   scratch; sync: 3 * (M / 16 + 2) ints, zero before the first call (the kernels leave them zero).  *fused_out tells whether the launch
   took the fused epilogue (N = 1024, every block resident at once); if not, X is updated and ln_out is left untouched. */
wm_status wm_op_gemm_resid_ln(int dtype, const void* A, const void* W, float* X, const float* bias, const float* gamma, const float* ln_w,
                              const float* ln_b, float ln_eps, void* ln_out, float* stats, int* sync, int M, int N, int K, int* fused_out,
                              void* stream);
/* Q must be pre-scaled by log2(e)/sqrt(64) (what wm_op_qkv_post does with q_scale): softmax is evaluated in base 2 */
wm_status wm_op_attention(int dtype, const void* Q, const void* K, const void* V, void* O, int H, int q_rows, int seq_len,
                          int kv_chunks, int kv_rows_per_chunk, void* stream);
/* Same with split-KV: kv_splits (1..4; 0 = choose) blocks per query tile each walk a slice of the keys and write
 * unnormalised partials into part_o (fp32 [kv_splits][q_rows][H*64]) and part_ml (fp32 [kv_splits][H][q_rows][2]);
 * a combine kernel finishes the softmax.  Used by the forward for cross-view attention when q-tiles x heads does
 * not fill the chip. */
wm_status wm_op_attention_split(int dtype, const void* Q, const void* K, const void* V, void* O, int H, int q_rows, int seq_len,
                                int kv_chunks, int kv_rows_per_chunk, int kv_splits, float* part_o, float* part_ml, void* stream);
/* The same with a flag workspace: unit_flags = int[wm_op_attention_flag_count(q_rows, seq_len, H)].  With it (bf16, whole
 * 64-key tiles, long sequences; selected by wm_set_tuning("attn_qb", 7) or the forward's own choice) the software-pipelined
 * kernel without a running max runs first and the general kernel recomputes the blocks it flagged (attention_v3.hip). */
wm_status wm_op_attention_ex(int dtype, const void* Q, const void* K, const void* V, void* O, int H, int q_rows, int seq_len,
                             int kv_chunks, int kv_rows_per_chunk, int kv_splits, float* part_o, float* part_ml, int* unit_flags,
                             void* stream);
size_t wm_op_attention_flag_count(int q_rows, int seq_len, int H);
/* prepare_splats' per-pixel assembly (src/models/models/rasterization.py:389-498, position_from = "gsdepth+predcamera"): gp [N*H*W][12]
 * raw head outputs, img [N][3][H][W], depth [N][H][W], cam [N][9] -> means / quats / scales / opacities / sh / weights */
wm_status wm_op_gs_splat(const float* gp, const float* img, const float* depth, const float* cam, float* means, float* quats,
                         float* scales, float* opac, float* sh, float* wts, int N, int H, int W, void* stream);
wm_status wm_op_layernorm(const float* x, void* y, const float* w, const float* b, int rows, int D, float eps, int out_f32,
                          int dtype, void* stream);
wm_status wm_op_qkv_post(int dtype, const float* qkv, void* q, void* k, void* v, const float* qn_w, const float* qn_b,
                         const float* kn_w, const float* kn_b, const float* rope_cos, const float* rope_sin, int M, int H,
                         int tokens_per_view, int patch_start, int grid_w, float q_scale, void* stream);
wm_status wm_op_conv(int dtype, const float* x, const void* w16, const float* bias, const float* resid, const float* resid2,
                     float* y, int N, int Hi, int Wi, int Cin, int Cout, int ksize, int stride, int pad, int relu_in,
                     int resid_relu, void* stream);
/* 3x3 / stride 1 / pad 1 conv of interpolate(x, (Hi, Wi), bilinear, align_corners=True) [+ separable position tables
 * addx [Wi][Cin/2], addy [Hi][Cin/2] or NULL], x NHWC [N][Hs][Ws][Cin]: the resize (dense_head.py:217-225) is fused
 * into the conv's input staging, the resized tensor is never stored.  Cin % 64 == 0, Cout % 4 == 0. */
wm_status wm_op_conv3x3_up(int dtype, const float* x, const void* w16, const float* bias, float* y, int N, int Hs, int Ws, int Hi, int Wi,
                           int Cin, int Cout, const float* addx, const float* addy, void* stream);
wm_status wm_op_bilinear(const float* in, float* out, int N, int Hi, int Wi, int Ho, int Wo, int C, void* stream);
wm_status wm_op_linear_f32(const float* X, const float* W, const float* b, float* Y, int M, int N, int K, int ldx, int pre_act,
                           int post_act, void* stream);

/* ---- operator-level entry points of the token front end and the camera head (parity tests: tests/test_gpu_ops_frontend.py).
 * Thin: they fill the launcher's arguments and map its status (WM_ERR_INVALID for a shape the launcher refuses, nothing launched). ---- */
/* Patchify (patch_embed.py:70, conv kernel = stride = ps as a GEMM): img f32 [N][C][H][W] -> out 16-bit [N*(H/ps)*(W/ps)][Kpad], column
 * c*ps*ps + ky*ps + kx, zeros in [C*ps*ps, Kpad); normalize (C = 3 only): (x - mean[c]) / std[c] of visual_transformer.py:16-17.
 * Rows and columns of the image beyond the last whole patch are dropped.  The launcher takes the input-indexed kernel when ps, W, C*ps*ps
 * and Kpad are even and ps * W * 2 bytes fit 64 KiB of LDS, the output-indexed one otherwise. */
wm_status wm_op_im2col(int dtype, const float* img, void* out, int N, int C, int H, int W, int ps, int Kpad, int normalize, void* stream);
/* im2col of Conv2d(3, C, 7, 1, 3) (dense_head.py:91-95): img f32 [N][3][H][W] -> out 16-bit [N*H*W][Kpad], column c*49 + ky*7 + kx, zeros
 * outside the image and in [147, Kpad) */
wm_status wm_op_im2col7(int dtype, const float* img, void* out, int N, int H, int W, int Kpad, void* stream);
/* Special rows of the DINO token buffer X f32 [N][1 + R + hw][D] (vision_transformer.py:215-219): row 0 = cls + pos[0], rows 1..R = reg;
 * the hw patch rows are not touched (patch is unused: the patch-embed GEMM writes them). */
wm_status wm_op_dino_tokens(const float* patch, const float* cls, const float* reg, const float* pos, float* X, int N, int hw, int R, int D,
                            void* stream);
/* Special rows [0, 1 + R + 2 cond) of the multi-view token buffer X f32 [N][P][D] (visual_transformer.py:285-295,397-416): cam_tok [2][D],
 * reg_tok [2][R][D] (slot 0 for GLOBAL view 0 = first_view_global + n, slot 1 for the others); with cond, rows 1 + R and 2 + R take
 * pose_tok [N][D] / ray_tok [N][D], or zeros where that pointer is NULL. */
wm_status wm_op_vgt_special(float* X, const float* cam_tok, const float* reg_tok, const float* pose_tok, const float* ray_tok, int N, int P,
                            int R, int D, int cond, int first_view_global, void* stream);
/* GEMM with the row-remapping epilogue: row r = g * rows_per_group + q of A W^T lands in C row g * out_group + out_off + q as
 * relu?(acc + bias) + add[q] (+ the old content when accumulate); add f32 [rows_per_group][N] or NULL; C f32, or 16-bit when out16 (no
 * accumulate); ldc in elements of C.  (patch embed + pos table, depth-prior MLP into the view tokens, the DPT heads' projections) */
wm_status wm_op_gemm_rowmap(int dtype, const void* A, const void* W, void* C, const float* bias, const float* add, int M, int N, int K,
                            int ldc, int rows_per_group, int out_group, int out_off, int accumulate, int out16, int relu, void* stream);
/* The front of the DPT heads for one tap (dense_head.py:53,204-208): out[k] [n hw][oc] = Linear_k(LayerNorm_k(tap patch rows)) + pos, for nheads
 * (1-4) heads reading the same tap f32 [n][P][D2] (patch rows psi .. psi + hw of every view); pos f32 [hw][oc] or NULL; out 16-bit when out16,
 * else f32.  norm_w / norm_b [D2], proj_w [oc][D2], proj_b [oc]: HOST fp32, one pointer per head; tap, pos, out[k]: device.
 * shared = 0: every head normalises with its own affine and projects (the forward with tuning tap_shared = 0).  shared = 1: the forward's default
 * form — one LayerNorm without affine, and ONE GEMM over the heads' weights W_k diag(norm_w_k) with bias proj_b_k + W_k norm_b_k (composed in
 * fp64, rounded once); when a composed weight is not finite in the operand type (or exceeds 65 504 for f16) the direct form runs instead.
 * *ran_shared (optional) tells which form ran.  Synchronises the stream (it owns scratch device memory). */
wm_status wm_op_dpt_tap_front(int dtype, const float* tap, int n, int P, int psi, int hw, int D2, int nheads, int oc,
                              const float* const* norm_w, const float* const* norm_b, const float* const* proj_w, const float* const* proj_b,
                              const float* pos, int out16, int shared, void* const* out, int* ran_shared, void* stream);
/* GEMM with the ConvTranspose2d(kernel = stride = ct_k) pixel-shuffle epilogue (dense_head.py:57-66): A 16-bit [n*ct_gh*ct_gw][K] tokens,
 * W 16-bit [ct_k*ct_k*ct_cout][K] with row (ii*ct_k + jj)*ct_cout + co, bias f32 [ct_cout] -> C f32 NHWC [n][ct_gh*ct_k][ct_gw*ct_k][ct_cout] */
wm_status wm_op_gemm_convt(int dtype, const void* A, const void* W, float* C, const float* bias, int M, int N, int K, int ct_k, int ct_cout,
                           int ct_gh, int ct_gw, void* stream);
/* LayerNorm with row remapping and row pitches: out row g*out_group + out_off + q <- in row g*in_group + in_off + q, q < rows_per_group,
 * g < groups; pitches ld_in / ld_out in elements (columns [D, ld_out) are not written); f32 or 16-bit output. */
wm_status wm_op_layernorm_rows(const float* x, void* y, const float* w, const float* b, int D, int ld_in, int ld_out, float eps, int groups,
                               int rows_per_group, int in_group, int in_off, int out_group, int out_off, int out_f32, int dtype, void* stream);
/* wm_op_bilinear + the separable position tables (dense_head.py:253-263): channel c < C/2 gets addx[x][c], the others addy[y][c - C/2]
 * (addx [Wo][C/2], addy [Ho][C/2], both or neither NULL); f32 output, and the same written as a 16-bit NHWC tensor */
wm_status wm_op_bilinear_add(const float* in, float* out, int N, int Hi, int Wi, int Ho, int Wo, int C, const float* addx, const float* addy,
                             void* stream);
wm_status wm_op_bilinear16(int dtype, const float* in, void* out16, int N, int Hi, int Wi, int Ho, int Wo, int C, const float* addx,
                           const float* addy, void* stream);
/* dst[r][0..cols) = src[r][0..cols), f32, row pitches ld_src / ld_dst (all multiples of 4) */
wm_status wm_op_copy2d(const float* src, float* dst, int rows, int cols, int ld_src, int ld_dst, void* stream);
/* Camera head (camera_head.py:84-147), all f32.  small_attention: qkv [S][3*heads*hd] -> out [S][heads*hd], softmax(q k^T / sqrt(hd)) v,
 * S <= 8192.  adaln: h = gate * (LayerNorm_noaffine(tok) * (1 + scale) + shift) + tok with mod [S][3*D] = (shift, scale, gate).
 * cam_update: pred [S][12] columns 0..8 = delta (first) or pred + delta, out [S][9] = the same with ReLU on columns 7, 8.
 * cam_matrices: params [S][9] = (t, quat xyzw, fov_h, fov_w) -> poses [S][4][4] = inverse of [R|t], intrs [S][3][3] (camera_utils.py:46-75). */
wm_status wm_op_small_attention(const float* qkv, float* out, int S, int heads, int hd, void* stream);
wm_status wm_op_adaln(const float* tok, const float* mod, float* h, int S, int D, float eps, void* stream);
wm_status wm_op_cam_update(float* pred, const float* delta, float* out, int S, int first, void* stream);
wm_status wm_op_cam_matrices(const float* params, float* poses, float* intrs, int S, int H, int W, void* stream);
/* wm_op_linear_f32 with the output pitch ldy, a per-column scale gamma (or NULL) and accumulation: Y (+)= gamma * post(pre(X) W^T + b) */
wm_status wm_op_linear_f32_ex(const float* X, const float* W, const float* b, float* Y, int M, int N, int K, int ldx, int ldy, int pre_act,
                              int post_act, const float* gamma, int accumulate, void* stream);
/* ---- operator-level entry points of the DPT heads' tails (parity tests: tests/test_gpu_ops_tails.py); thin, as the ones above ---- */
/* The tail of a DPT head (src/models/heads/dense_head.py:97-105 output_conv2[1:], :297-344 activate_head, :356 the inverse log transform):
 * y32 f32 [npix][32] -> ReLU -> 1x1 conv 32 -> C (w f32 [C][32], b f32 [C]) -> attr f32 [npix][C - 1] = act(first C - 1 channels),
 * conf f32 [npix] = 1 + exp(last channel).  act: 0 = inv_log (sign(x) expm1(|x|)), 1 = exp, 2 = norm (x / |x|, no epsilon: the zero vector
 * gives NaN as in the reference).  C in 2..4, anything else is WM_ERR_INVALID.  NaN in y32, w or b reaches every output it feeds. */
wm_status wm_op_dpt_tail(const float* y32, const float* w, const float* b, float* attr, float* conf, size_t npix, int C, int act, void* stream);
/* wm_op_up_conv_n32 (below) with that tail in the conv's epilogue (dense_head.py:217-251 + the lines above): the launch pair the forward
 * makes for the depth / pts / normal heads when dpt_features / 2 is a multiple of 64; the 32-channel tensor is never stored.  tail_w f32
 * [tail_C][32], tail_b f32 [tail_C], tail_C in 2..4, tail_act as act above, attr f32 [N][Hi][Wi][tail_C - 1], conf f32 [N][Hi][Wi]; Cin 64
 * or 128; up16 as for wm_op_up_conv_n32 (it holds the rounded resize afterwards). */
wm_status wm_op_up_conv_n32_tail(int dtype, const float* x, const void* w16, const float* bias, int N, int Hs, int Ws, int Hi, int Wi, int Cin,
                                 const float* addx, const float* addy, const float* tail_w, const float* tail_b, int tail_C, int tail_act,
                                 float* attr, float* conf, void* up16, void* stream);
/* ---- post-path geometry (the step right after the path in infer.py:303 / app.py:151) ----
 * depth_to_world_coords_points (src/models/utils/geometry.py:57-89): depth [B][H][W] f32, extrinsic [B][4][4]
 * camera-to-world, intrinsic [B][3][3] -> world [B][H][W][3], cam [B][H][W][3], mask [B][H][W] (u8, depth > eps).
 * Any of world / cam / mask may be NULL.  Device pointers, stream-ordered. */
wm_status wm_depth_to_world(const float* depth, const float* extrinsic, const float* intrinsic, float* world, float* cam,
                            unsigned char* mask, int B, int H, int W, float eps, void* stream);

/* ---- image ingest after decode ----
 * load_and_preprocess_images (src/utils/inference_utils.py:67-108) for ONE decoded image: rgb [H][W][3] uint8 (device)
 * -> Pillow-exact BICUBIC resize to (518, round(H*518/W/14)*14) ["crop", mode 0] or the longer side to 518 ["pad",
 * mode 1] -> /255 -> centre crop of the height / white padding to the square -> out planar float32 [3][out_h][out_w]
 * (device; sizes from wm_preprocess_image_size).  Decoding, alpha compositing and stacking stay on the host side of
 * the binding.  workspace: wm_preprocess_image_workspace_bytes bytes of device memory. */
wm_status wm_preprocess_image_size(int H, int W, int mode, int output_size, int* out_h, int* out_w);
size_t wm_preprocess_image_workspace_bytes(int H, int W, int mode, int output_size);
wm_status wm_preprocess_image(const unsigned char* rgb, int H, int W, int mode, int output_size, float* out, void* workspace,
                              size_t workspace_bytes, void* stream);

/* create_confidence_mask (infer.py:25-59): mask[i] = 1 for the top ceil(n (100 - p) / 100) (at least 1; p <= 0: all)
 * confidences after conf <= 1e-5 -> -inf; the count is taken in double from the double p, as the reference takes it from its Python
 * float.  A NaN of either sign ranks above +inf (torch.topk's order); all NaNs tie.  Exact radix select on the device, ties at the
 * threshold value broken by lowest index (the reference's torch.topk leaves them unspecified).  workspace:
 * wm_confidence_mask_workspace_bytes(n) bytes of device memory.  n < 2^32.  A NULL conf, mask or workspace, or a workspace smaller
 * than that, returns WM_ERR_INVALID before anything is launched. */
size_t wm_confidence_mask_workspace_bytes(size_t n);
wm_status wm_confidence_mask(const float* conf, size_t n, double conf_threshold_percent, unsigned char* mask, void* workspace,
                             size_t workspace_bytes, void* stream);
/* The same select with the count given instead of a percentage: mask[i] = 1 for the k highest confidences, 1 <= k <= n, all other rules
 * (conf <= 1e-5 -> -inf, NaN above +inf, ties to the lowest indices) and the workspace as above.  It serves
 * GaussianSplatRenderer.apply_confidence_filter (src/models/models/rasterization.py:248-299), whose count is capped by max_gaussians.
 * WM_ERR_INVALID, before anything is launched: a NULL pointer, n < 1, k outside 1..n, n >= 2^32, a too small workspace. */
wm_status wm_confidence_mask_count(const float* conf, size_t n, size_t k, unsigned char* mask, void* workspace, size_t workspace_bytes,
                                   void* stream);

/* ---- novel-view path: the target-view validity mask (csrc/frustum.hip; reference: src/models/utils/frustum.py:26-89
 * calculate_in_frustum_mask).  depth_1 [B][V1][H][W] (target views) and depth_2 [B][V2][H][W] (context views) contiguous fp32;
 * kinv_1 [B][V1][3][3] = K1^-1; rel [B][V1][V2][3][4] = rows 0..2 of c2w_2[b][j]^-1 c2w_1[b][i]; k_2 [B][V2][3][3].  The caller takes the
 * inverses once (the Python binding does, in fp64); the per-pixel arithmetic is fp32, the division by z one hardware reciprocal (1 ulp).
 * mask [B][V1][H][W] u8:
 *   mask = any_j(0 < px_j < W && 0 < py_j < H) && depth_1 > 1e-6 && any_j(isclose(z_j, sample_j, atol = 0.1, rtol = 1e-5))
 * for (px_j, py_j, z_j) the pixel's point projected into context view j (divided by z without a z > 0 test, as the reference) and
 * sample_j the bilinear, zero-padded sample of depth_2[b][j] at (px_j - 0.5, py_j - 0.5) (grid_sample, align_corners = False); a NaN on
 * either side of the comparison gives false; the two any are independent.  One kernel, no workspace, no atomics: the same bits on
 * every run.  Device pointers, stream-ordered.  WM_ERR_INVALID, before anything is launched: a NULL pointer, a size < 1,
 * B V1 H W or B V2 H W >= 2^31, B V1 V2 >= 2^24. */
wm_status wm_in_frustum_mask(const float* depth_1, const float* depth_2, const float* kinv_1, const float* rel, const float* k_2, int B,
                             int V1, int V2, int H, int W, unsigned char* mask, void* stream);

/* Point-cloud filter masks: the per-view mask app.py:172-206 (run_model) builds for every export.
 * All views are S x H x W, S*H*W < 2^31; k (window) is 3, 5 or 7; outputs are u8 0/1.  Bit-for-bit semantics of the
 * reference's numpy code, including its transposed mask window in normals_edge and its NaN handling (pointmask.hip).
 * depth_edge (src/utils/geometry.py:374-416): depth [S][H][W] f32, mask [S][H][W] u8 or NULL; atol / rtol apply when
 * has_atol / has_rtol (compared in fp32, as numpy 2 compares a Python float against a float32 array). */
wm_status wm_depth_edge(const float* depth, const unsigned char* mask, int S, int H, int W, int k, int has_atol, float atol,
                        int has_rtol, float rtol, unsigned char* out, void* stream);
/* normals_edge (src/utils/geometry.py:472-531): normals [S][H][W][3] f32, mask [S][H][W] u8 or NULL (with a mask, each view
 * is the reference's 2-D call); tol in degrees (edge: fp64 angle > np.deg2rad(tol)). */
wm_status wm_normals_edge(const float* normals, const unsigned char* mask, int S, int H, int W, int k, double tol_deg, unsigned char* out,
                          void* stream);
/* app.py:172-206 in one call: per view, conf_mask = conf >= np.quantile(conf[i], percentile / 100) (apply_conf; numpy's linear
 * method, exact), then conf_mask & ~(depth_edge(depth[i], rtol=depth_rtol, mask) & normals_edge(normals[i], normal_tol_deg, mask))
 * (apply_edge; mask = conf_mask or NULL, k = 3); neither flag: all ones.  conf / depth [S][H][W] f32, normals [S][H][W][3] f32,
 * mask_out [S][H][W] u8, thresholds_out [S] f32 (the per-view np.quantile values; may be NULL).  workspace:
 * wm_point_filter_mask_workspace_bytes(S, H, W) bytes of device memory. */
size_t wm_point_filter_mask_workspace_bytes(int S, int H, int W);
wm_status wm_point_filter_mask(const float* conf, const float* depth, const float* normals, int S, int H, int W, int apply_conf,
                               double percentile, int apply_edge, double normal_tol_deg, float depth_rtol, float* thresholds_out,
                               unsigned char* mask_out, void* workspace, size_t workspace_bytes, void* stream);

/* Operator-level entry (parity tests / A-B): F.interpolate(x, (Hi, Wi), bilinear, align_corners=True) (+ separable position tables
 * addx [Wi][Cin/2], addy [Hi][Cin/2], may be NULL) rounded to the 16-bit operand type, then Conv2d(Cin, 32, 3, padding=1) (+ ReLU):
 * the un-fused form the DPT tail uses for output_conv2[0] (dense_head.py:97-105,217-251).  up16: caller-owned device scratch of
 * N*Hi*Wi*Cin 16-bit elements + 32 bytes. */
wm_status wm_op_up_conv_n32(int dtype, const float* x, const void* w16, const float* bias, float* y, int N, int Hs, int Ws, int Hi,
                            int Wi, int Cin, const float* addx, const float* addy, int relu_out, void* up16, void* stream);

/* Operator-level entry (parity tests / A-B): wm_op_conv's 3x3 / stride 1 / pad 1 case with the 16-bit tensor forms the DPT heads use
 * between their convs (dense_head.py:435-455): x is a 16-bit NHWC tensor of the operand type when in16 (relu_in must be 0: the producer
 * applied it), y is one when out16 (+ ReLU when relu_out).  WM_ERR_INVALID when the shape's kernel has no such form. */
wm_status wm_op_conv_ex(int dtype, const void* x, int in16, const void* w16, const float* bias, const float* resid, const float* resid2,
                        void* y, int out16, int N, int Hi, int Wi, int Cin, int Cout, int relu_in, int resid_relu, int relu_out, void* stream);

/* Operator-level entry (parity tests / A-B): Conv2d(Cm, 256, 3, padding=1, bias=False)(ConvTranspose2d(Cin, Cm, k, stride=k)(tokens)) — the DPT
 * head's resize_layers[0 / 1] followed by scratch.layer{1,2}_rn (dense_head.py:57-66,196-214,277-278,394-399) — composed into ONE block-sparse GEMM
 * at the token resolution: per output phase the 3x3 taps land in at most 2 x 2 neighbouring tokens, so 36 (k = 4) / 16 (k = 2) combined
 * matrices replace k^2 x 9 tap products per token.  tokens16: device, 16-bit NHWC [N][gh][gw][Cin]; wct [Cin][Cm][k][k], bct [Cm], wrn
 * [256][Cm][3][3]: HOST fp32, torch layouts (combined in fp32 on the device, rounded once); out: device fp32 NHWC [N][k*gh][k*gw][256];
 * zero16: >= 128 B of device zeros.  k in {2, 4}; Cin % 64 == 0.  Synchronises the stream (it builds and frees the combined weights). */
wm_status wm_op_tconv(int dtype, const void* tokens16, const float* wct, const float* bct, const float* wrn, float* out, int N, int gh, int gw,
                      int k, int Cin, int Cm, const void* zero16, void* stream);

/* Operator-level entry (parity tests / A-B): Conv2d(C, Co, 3, padding=1)(F.interpolate(x, (Ho, Wo), mode="bilinear", align_corners=True)) —
 * the DPT head's output_conv1 behind its last resize (dense_head.py:217-225,265-295) — in the tap form: the nine 1x1 products W_tap x at the
 * LOW resolution (one GEMM, a quarter of the direct conv's flops) and a bilinear gather of them.  x16: f16 NHWC [N][Hi][Wi][C]; w16:
 * [Co][3][3][C]; out: fp32 NHWC [N][Ho][Wo][Co]; wt16 / y16: caller-owned device scratch of 9*Co*C and N*Hi*Wi*9*Co 16-bit elements.
 * dtype must be f16 (the products are stored in the operand type); C % 64 == 0; Co in {32, 64, 128}. */
wm_status wm_op_upconv3x3_tap(int dtype, const void* x16, const void* w16, const float* bias, float* out, int N, int Hi, int Wi, int Ho,
                              int Wo, int C, int Co, void* wt16, void* y16, void* stream);

/* The gather half of wm_op_upconv3x3_tap on its own (timing tools): y16 f16 [N][Hi][Wi][9][Co] -> out fp32 [N][Ho][Wo][Co] (+ bias). */
wm_status wm_op_upconv_gather(const void* y16, const float* bias, float* out, int N, int Hi, int Wi, int Ho, int Wo, int Co, void* stream);

/* Operator-level entry (parity tests / A-B): Conv2d(Cin, Cout, 3, padding=1) on a 16-BIT NHWC tensor x16 [N][H][W][Cin] of the operand
 * type, run as the ping-pong GEMM itself (rows = pixels, K = (tap, channel); no im2col): y = conv(x16) + bias + relu?(resid) + resid2,
 * optional ReLU; y is fp32 NHWC, or 16-bit NHWC when out16.  The form the ResidualConvUnit's second conv takes (dense_head.py:435-455)
 * when tuning "conv_gemm" = 1.  zero16: >= 128 B of device zeros.  Cin % 64 == 0, Cout % 8 == 0. */
wm_status wm_op_conv3x3_gemm16(int dtype, const void* x16, const void* w16, const float* bias, const float* resid, int resid_relu,
                               const float* resid2, void* y, int out16, int relu_out, int N, int H, int W, int Cin, int Cout,
                               const void* zero16, void* stream);

/* Voxel merge of the per-pixel splats — GaussianSplatRenderer.prune_gs (src/models/models/rasterization.py:301-387; called at
 * :216 and on predictions["splats"] by the callers).  Inputs [n, ...] device fp32: means [n,3], quats [n,4], scales [n,3],
 * opacities [n] (not read: the merged opacity is sum w^2 / sum w, as in the reference), sh [n,3] (degree-0 coefficients), weights [n].
 * Outputs have room for n rows; *n_voxels (host) = occupied voxels K, rows [0, K) are valid and ordered by ascending voxel
 * index (torch.unique's order).  Sums run in original index order, i.e. bit-identical to the reference on CPU.  One stream
 * synchronisation (K is data dependent). */
size_t wm_prune_gs_workspace_bytes(size_t n);
wm_status wm_prune_gs(const float* means, const float* quats, const float* scales, const float* opacities, const float* sh,
                      const float* weights, int n, float voxel_size, float* out_means, float* out_quats, float* out_scales,
                      float* out_opacities, float* out_sh, int* n_voxels, void* workspace, size_t workspace_bytes, void* stream);

/* 3D-Gaussian-splat rasteriser forward — replaces gsplat.rasterization as the reference calls it through
 * Rasterizer.rasterize_splats (src/models/models/rasterization.py:29-66; callers: GaussianSplatRenderer.render :221-241,
 * render_interpolated_video src/utils/render_utils.py:242-312 <- infer.py:264): packed, rasterize_mode "classic", pinhole,
 * render_mode "RGB+ED" (colour + expected depth), tile size 16, eps2d 0.3, near plane 0.01, no background.
 * means [N,3], quats [N,4] (wxyz, normalised inside), scales [N,3], opacities [N], colors [N,3]: degree-0 SH coefficients
 * (colors_are_sh0 = 1: colour = max(0.2820948 sh + 0.5, 0), the reference's sh_degree = 0 call) or final colours (0: the
 * reference's sh_degree = None call); viewmats [C,4,4] WORLD-TO-CAMERA (the reference inverts its camtoworlds before the
 * call, :48), Ks [C,3,3].  Outputs (caller-owned device buffers): out_rgb [C,H,W,3], out_depth [C,H,W] (expected depth
 * = sum w z / sum w), out_alpha [C,H,W]; radii_out optional [C,N,2] int32 (the projection's screen radii, 0 = culled).
 * The number of (Gaussian, tile) pairs is data dependent: the call synchronises the stream once to read it (as the
 * reference's isect_tiles does); if it exceeds max_isects the call returns WM_ERR_STATE with *n_isects = the required count
 * and renders nothing — re-size the workspace with wm_rasterize_workspace_bytes and call again. */
size_t wm_rasterize_workspace_bytes(int n_gaussians, int n_cameras, int width, int height, size_t max_isects);
wm_status wm_rasterize_splats(const float* means, const float* quats, const float* scales, const float* opacities,
                              const float* colors, int colors_are_sh0, int n_gaussians, const float* viewmats, const float* Ks,
                              int n_cameras, int width, int height, float* out_rgb, float* out_depth, float* out_alpha,
                              int* radii_out, void* workspace, size_t workspace_bytes, size_t max_isects,
                              unsigned long long* n_isects, void* stream);

/* 3D-Gaussian-splat rasteriser backward — the gradient gsplat.rasterization gives through its autograd functions
 * (gsplat/cuda/_wrapper.py _RasterizeToPixels.backward -> csrc/RasterizeToPixels3DGSBwd.cu, _FullyFusedProjection.backward,
 * _QuatScaleToCovarPreci.backward), which the reference's "Post 3DGS Optimization" (README; gsplat's simple_trainer) runs on.
 * Gradients of out_rgb / out_depth / out_alpha of ONE wm_rasterize_splats call with respect to means [N,3], quats [N,4] (through
 * the normalisation), scales [N,3], opacities [N] and colors [N,3] (the degree-0 SH coefficients when colors_are_sh0: zero where
 * 0.2820948 sh + 0.5 <= 0).  No packed / sparse layout; the 2-D mean gradient and absgrad: the _ex entry below; the gradient for
 * viewmats: the _cam entry below; none for Ks.
 * CONTRACT: pass the same inputs, sizes, workspace, workspace_bytes and max_isects as the forward call and the *n_isects it
 * reported; the workspace must be UNTOUCHED between that forward and this call (no other wm_rasterize_splats on it): the
 * backward reads the projection records, the sorted pair list and the tile offsets the forward left there.  out_depth is the
 * forward's output; out_rgb and out_alpha are part of the interface but are not read (may be null).  v_rgb [C,H,W,3], v_depth
 * [C,H,W], v_alpha [C,H,W]: cotangents.  All five gradient outputs are overwritten (zero for Gaussians no camera sees).
 * grad_workspace: wm_rasterize_backward_workspace_bytes bytes (40 bytes per (Gaussian, tile) pair).  Sums run in a fixed
 * order, no atomics: results are bitwise reproducible.  Asynchronous on stream.  Returns WM_ERR_STATE when n_isects >
 * max_isects (that forward rendered nothing), WM_ERR_INVALID / WM_ERR_HIP as the forward. */
size_t wm_rasterize_backward_workspace_bytes(int n_gaussians, int n_cameras, int width, int height, size_t n_isects);
wm_status wm_rasterize_splats_backward(const float* means, const float* quats, const float* scales, const float* opacities,
                                       const float* colors, int colors_are_sh0, int n_gaussians, const float* viewmats, const float* Ks,
                                       int n_cameras, int width, int height, const void* workspace, size_t workspace_bytes,
                                       size_t max_isects, size_t n_isects, const float* out_rgb, const float* out_depth,
                                       const float* out_alpha, const float* v_rgb, const float* v_depth, const float* v_alpha,
                                       float* v_means, float* v_quats, float* v_scales, float* v_opacities, float* v_colors,
                                       void* grad_workspace, size_t grad_workspace_bytes, void* stream);

/* The same backward with what a densification strategy reads (gsplat: info["means2d"].grad / .absgrad, strategy/default.py:220-226).
 * Arguments and the five gradients as wm_rasterize_splats_backward, bit for bit; in addition
 *   v_means2d     [C,N,2] optional: gradient of the pixel-space means, per (camera, Gaussian) the sum over its tiles of the tiles'
 *                 sums; zero where the camera culled the Gaussian.
 *   v_means2d_abs [C,N,2], required with want_absgrad = 1 (then v_means2d is required too): over all pixels that blended the pair,
 *                 the sum of the ABSOLUTE value of the pixel's two 2-D mean terms, taken per pixel before any sum (gsplat's
 *                 absgrad, RasterizeToPixels3DGSBwd.cu); zero where culled.  Not written with want_absgrad = 0.
 * grad_workspace: wm_rasterize_backward_workspace_bytes_ex bytes: 40 bytes per (Gaussian, tile) pair, 48 with want_absgrad.
 * Fixed summation order, no atomics, bitwise reproducible; v_means2d is the same bits with and without want_absgrad. */
size_t wm_rasterize_backward_workspace_bytes_ex(int n_gaussians, int n_cameras, int width, int height, size_t n_isects, int want_absgrad);
wm_status wm_rasterize_splats_backward_ex(const float* means, const float* quats, const float* scales, const float* opacities,
                                          const float* colors, int colors_are_sh0, int n_gaussians, const float* viewmats, const float* Ks,
                                          int n_cameras, int width, int height, const void* workspace, size_t workspace_bytes,
                                          size_t max_isects, size_t n_isects, const float* out_rgb, const float* out_depth,
                                          const float* out_alpha, const float* v_rgb, const float* v_depth, const float* v_alpha,
                                          float* v_means, float* v_quats, float* v_scales, float* v_opacities, float* v_colors,
                                          float* v_means2d, float* v_means2d_abs, int want_absgrad,
                                          void* grad_workspace, size_t grad_workspace_bytes, void* stream);
/* The same backward with the gradient of the cameras — replaces the viewmats gradient of gsplat's _FullyFusedProjection.backward
 * (gsplat/cuda/_wrapper.py; restated in _torch_impl.py:250-283 _world_to_cam), which the reference's post-3DGS trainer feeds to its
 * CameraOptModule under --pose_opt (simple_trainer_worldmirror.py:511-523, 734-735, 948-950).
 * Arguments as wm_rasterize_splats_backward_ex (v_means2d / v_means2d_abs optional in the same way) plus
 *   v_viewmats [C,4,4], required: gradient with respect to the WORLD-TO-CAMERA matrices, [c,:3,:3] = v_R, [c,:3,3] = v_t, where per
 *              visible (camera, Gaussian) pair v_t += v_mean_camera and v_R += outer(v_mean_camera, mean) + (v_S + v_S^T) R cov.
 *              Overwritten; exact zeros in every bottom row and for a camera that sees nothing.  Ks gets no gradient, as in gsplat.
 * The five splat gradients (and v_means2d, v_means2d_abs) equal those of the entries above bit for bit.
 * Summation order: the per-pair terms are fp32; from there on fp64: each 64-Gaussian wave sums its lanes by a fixed butterfly, then per
 * (camera, component) the waves' partials are added in a fixed order (256 strided running sums, then a fixed pairwise tree) and the
 * result is rounded to fp32 once.  No atomics, bitwise reproducible; nothing depends on what grad_workspace held before.
 * grad_workspace: wm_rasterize_backward_workspace_bytes_cam bytes = the _ex size + 96 bytes per camera per 64 Gaussians (rounded up
 * to 256); a smaller workspace returns WM_ERR_INVALID before anything is launched. */
size_t wm_rasterize_backward_workspace_bytes_cam(int n_gaussians, int n_cameras, int width, int height, size_t n_isects, int want_absgrad);
wm_status wm_rasterize_splats_backward_cam(const float* means, const float* quats, const float* scales, const float* opacities,
                                           const float* colors, int colors_are_sh0, int n_gaussians, const float* viewmats, const float* Ks,
                                           int n_cameras, int width, int height, const void* workspace, size_t workspace_bytes,
                                           size_t max_isects, size_t n_isects, const float* out_rgb, const float* out_depth,
                                           const float* out_alpha, const float* v_rgb, const float* v_depth, const float* v_alpha,
                                           float* v_means, float* v_quats, float* v_scales, float* v_opacities, float* v_colors,
                                           float* v_means2d, float* v_means2d_abs, int want_absgrad, float* v_viewmats,
                                           void* grad_workspace, size_t grad_workspace_bytes, void* stream);
/* View-dependent colour: the forward with real spherical harmonics of degree 1-3 — replaces gsplat.rasterization called with
 * colors [N,K,3] and sh_degree > 0 (gsplat/rendering.py:509-525 -> gsplat/cuda/_wrapper.py spherical_harmonics, restated in
 * _torch_impl.py:720-822), which the reference's post-3DGS trainer selects as sh_degree_to_use rises (simple_trainer_worldmirror.py:613,
 * :738-746).  Arguments as wm_rasterize_splats, with in place of colors / colors_are_sh0:
 *   sh_coeffs [N,n_coeffs,3], sh_degree L in 1..3 with (L + 1)^2 <= n_coeffs (bands at or above (L + 1)^2 are not read),
 *   campos [C,3]: the cameras' world positions (gsplat: inverse(viewmats)[:, :3, 3]).
 * Per (camera, Gaussian) pair that the projection did not cull: colour = max(sum_k B_k(normalize(means - campos)) sh_coeffs[k] + 0.5, 0),
 * normalize(d) = d / max(|d|, 1e-12).  Projection, binning, sort and compositing are those of wm_rasterize_splats; the workspace is
 * wm_rasterize_workspace_bytes.  WM_ERR_INVALID for L < 1, L > 3 or (L + 1)^2 > n_coeffs; WM_ERR_STATE as wm_rasterize_splats. */
wm_status wm_rasterize_splats_sh(const float* means, const float* quats, const float* scales, const float* opacities,
                                 const float* sh_coeffs, int n_coeffs, int sh_degree, const float* campos, int n_gaussians,
                                 const float* viewmats, const float* Ks, int n_cameras, int width, int height, float* out_rgb,
                                 float* out_depth, float* out_alpha, int* radii_out, void* workspace, size_t workspace_bytes,
                                 size_t max_isects, unsigned long long* n_isects, void* stream);
/* Backward of ONE wm_rasterize_splats_sh call — replaces the backward of gsplat's _SphericalHarmonics (gsplat/cuda/_wrapper.py; gradient
 * to the coefficients and, through dirs = means - campos, to the means and the cameras) together with what wm_rasterize_splats_backward_cam
 * replaces.  Same CONTRACT on the forward's workspace as wm_rasterize_splats_backward.  Outputs, a superset of the _cam entry's:
 *   v_means, v_quats, v_scales, v_opacities   as the entries above; v_means includes the colour's term through the direction
 *   v_sh_coeffs [N,n_coeffs,3]                sum over cameras of B_k v_colour, v_colour zero where the clamped channel is 0; bands at or
 *                                             above (L + 1)^2 are written as exact zeros
 *   v_means2d, v_means2d_abs, want_absgrad    optional, as the _ex entry
 *   v_viewmats [C,4,4]                        optional (may be null), as the _cam entry: the PROJECTION's term only, bottom row exact zeros
 *   v_campos [C,3]                            optional (may be null): the colour's camera term, minus the sum over Gaussians of the
 *                                             direction's gradient; exact zeros for a camera that sees nothing
 * v_campos is summed as v_viewmats is: per-pair terms fp32, from there on fp64, a fixed butterfly over each wave's 64 lanes, the waves'
 * partials added in a fixed order, rounded to fp32 once.  No atomics, bitwise reproducible; nothing depends on what grad_workspace held.
 * grad_workspace: wm_rasterize_backward_workspace_bytes_sh bytes (the _ex / _cam size + 12 bytes per Gaussian, + 24 bytes per camera per
 * 64 Gaussians with want_campos, each rounded up to 256); a smaller one returns WM_ERR_INVALID before anything is launched. */
size_t wm_rasterize_backward_workspace_bytes_sh(int n_gaussians, int n_cameras, int width, int height, size_t n_isects, int want_absgrad,
                                                int want_viewmats, int want_campos);
wm_status wm_rasterize_splats_backward_sh(const float* means, const float* quats, const float* scales, const float* opacities,
                                          const float* sh_coeffs, int n_coeffs, int sh_degree, const float* campos, int n_gaussians,
                                          const float* viewmats, const float* Ks, int n_cameras, int width, int height,
                                          const void* workspace, size_t workspace_bytes, size_t max_isects, size_t n_isects,
                                          const float* out_rgb, const float* out_depth, const float* out_alpha, const float* v_rgb,
                                          const float* v_depth, const float* v_alpha, float* v_means, float* v_quats, float* v_scales,
                                          float* v_opacities, float* v_sh_coeffs, float* v_means2d, float* v_means2d_abs,
                                          int want_absgrad, float* v_viewmats, float* v_campos, void* grad_workspace,
                                          size_t grad_workspace_bytes, void* stream);
/* gsplat.rasterization's own options — replaces the keyword arguments the reference's post-3DGS trainer passes to gsplat.rasterization
 * (simple_trainer_worldmirror.py:619-642, :741-752; gsplat/rendering.py): rasterize_mode, near_plane / far_plane, eps2d, radius_clip,
 * backgrounds and the depth half of render_mode.  A null options pointer means the defaults noted beside the fields, which are what the
 * entries above render. */
typedef struct wm_raster_options {
  int   antialiased;    /* 0 classic, 1: opacity * sqrt(max(det(cov2d) / det(cov2d + eps2d I), 0)) (_torch_impl.py:329-344) */
  int   depth_mode;     /* 0 expected (ED): sum w z / max(alpha, 1e-10); 1 accumulated (D): sum w z (rendering.py:984-992) */
  float eps2d;          /* 0.3: the blur added to the 2-D covariance's diagonal (not the 0.3 of _persp_proj's clamp limits) */
  float near_plane;     /* 0.01 */
  float far_plane;      /* 1e10 */
  float radius_clip;    /* 0: a (camera, Gaussian) pair whose two radii are both <= radius_clip pixels is culled (gsplat's
                           ProjectionEWA3DGSFused.cu; 0 culls nothing) */
  const float* backgrounds;  /* device [C,3] or null: out_rgb += backgrounds[c] (1 - alpha); the depth channel gets none (rendering.py:926-939) */
} wm_raster_options;
/* The forward with options: a superset of wm_rasterize_splats and wm_rasterize_splats_sh.  Colours in either form: sh_degree = 0 with
 * colors [N,3] and colors_are_sh0 as wm_rasterize_splats (n_coeffs, campos not read), or sh_degree 1-3 with colors = sh_coeffs
 * [N,n_coeffs,3] and campos [C,3] as wm_rasterize_splats_sh (colors_are_sh0 not read).  Outputs, workspace (wm_rasterize_workspace_bytes),
 * max_isects / *n_isects and WM_ERR_STATE exactly as wm_rasterize_splats; wm_rasterize_means2d works on the workspace this call leaves.
 * out_depth holds the depth channel of the chosen depth_mode.  WM_ERR_INVALID, before anything is launched, for eps2d < 0,
 * near_plane >= far_plane, radius_clip < 0, depth_mode or antialiased outside {0, 1}, sh_degree outside 0..3, (sh_degree + 1)^2 > n_coeffs
 * or a null campos with sh_degree > 0.  With null (default) options the outputs are those of the entries above, bit for bit.
 * Per-camera colours: colors_are_sh0 = WM_COLORS_PER_CAMERA makes colors [C,N,3], post-activation colours with a camera axis (one of the
 * colour shapes gsplat.rasterization takes with sh_degree = None, gsplat/rendering.py's colour handling ahead of the SH branch at :509-525;
 * the reference trainer's --app_opt passes sigmoid(app_module(...) + colors), simple_trainer_worldmirror.py:603-611): the pair (c, g) is
 * rendered with colors[c,g,:] as it is (no + 0.5, no clamp); n_coeffs and campos are not read and sh_degree must be 0.  The backward's
 * v_colors is then [C,N,3]: per pair the sum of its tiles' colour terms, exact zeros where the camera culled the Gaussian, every slot
 * written.  All other outputs and the workspace sizes are those of colors [N,3].  WM_ERR_INVALID, before anything is launched, for
 * colors_are_sh0 outside {0, 1, 2} and for WM_COLORS_PER_CAMERA with sh_degree > 0. */
#ifndef WM_COLORS_PER_CAMERA
#define WM_COLORS_PER_CAMERA 2
#endif
wm_status wm_rasterize_splats_opt(const float* means, const float* quats, const float* scales, const float* opacities,
                                  const float* colors, int colors_are_sh0, int n_coeffs, int sh_degree, const float* campos,
                                  int n_gaussians, const float* viewmats, const float* Ks, int n_cameras, int width, int height,
                                  const wm_raster_options* options, float* out_rgb, float* out_depth, float* out_alpha,
                                  int* radii_out, void* workspace, size_t workspace_bytes, size_t max_isects,
                                  unsigned long long* n_isects, void* stream);
/* Backward of ONE wm_rasterize_splats_opt call (same options, same CONTRACT on the forward's workspace as wm_rasterize_splats_backward) —
 * replaces what gsplat's autograd gives for the options: the compensation's gradient (gsplat/cuda/include/Utils.cuh add_blur_vjp), the
 * background term of rendering.py:926-939 and the depth mode's.  Outputs: all of the _sh entry's (v_colors [N,3], or [N,n_coeffs,3] with
 * sh_degree > 0; v_means2d, v_means2d_abs, v_viewmats, v_campos optional; v_campos needs sh_degree > 0) plus
 *   v_backgrounds [C,3] optional (needs options->backgrounds and out_alpha, the forward's alpha, which is READ): sum over the camera's
 *                 pixels of v_rgb (1 - alpha).  Terms fp32; from there on fp64: per 4096-pixel chunk 256 strided running sums and a fixed
 *                 pairwise tree, then the chunks' partials in a fixed order (256 strided running sums, a fixed tree), rounded to fp32 once.
 * Antialiased: v_opacities = sum over cameras of comp * v_opacity'; v_comp = opacity * v_opacity' enters the 2-D covariance's gradient with
 * the EXACT derivative 0.5 / comp (autograd's on the torch projection; gsplat's CUDA divides by comp + 1e-6), exactly 0 where comp == 0 or
 * the determinant clamp is active (never NaN).  Accumulated depth: v_depth is the cotangent of sum w z itself.  Everything else: summation
 * order, no atomics, bitwise reproducible, as the entries above; with null options the same bits as those entries.
 * grad_workspace: wm_rasterize_backward_workspace_bytes_opt bytes = the _sh / _cam / _ex size for the same requests (sh_degree > 0 adds the
 * _sh parts) + with want_backgrounds 24 bytes per camera per 4096 pixels (rounded up to 256); a smaller one returns WM_ERR_INVALID before
 * anything is launched, as do invalid options. */
size_t wm_rasterize_backward_workspace_bytes_opt(int n_gaussians, int n_cameras, int width, int height, size_t n_isects, int want_absgrad,
                                                 int want_viewmats, int sh_degree, int want_campos, int want_backgrounds);
wm_status wm_rasterize_splats_backward_opt(const float* means, const float* quats, const float* scales, const float* opacities,
                                           const float* colors, int colors_are_sh0, int n_coeffs, int sh_degree, const float* campos,
                                           int n_gaussians, const float* viewmats, const float* Ks, int n_cameras, int width, int height,
                                           const wm_raster_options* options, const void* workspace, size_t workspace_bytes,
                                           size_t max_isects, size_t n_isects, const float* out_rgb, const float* out_depth,
                                           const float* out_alpha, const float* v_rgb, const float* v_depth, const float* v_alpha,
                                           float* v_means, float* v_quats, float* v_scales, float* v_opacities, float* v_colors,
                                           float* v_means2d, float* v_means2d_abs, int want_absgrad, float* v_viewmats, float* v_campos,
                                           float* v_backgrounds, void* grad_workspace, size_t grad_workspace_bytes, void* stream);
/* The pixel-space means [C,N,2] of ONE wm_rasterize_splats call, read out of the workspace it left (same sizes and max_isects,
 * workspace untouched since); radii: that call's radii_out.  Zero where a radius is 0 (culled).  Asynchronous on stream. */
wm_status wm_rasterize_means2d(const void* workspace, size_t workspace_bytes, int n_gaussians, int n_cameras, int width, int height,
                               size_t max_isects, const int* radii, float* means2d, void* stream);

/* Splat densification: gsplat's DefaultStrategy (gsplat/strategy/default.py, ops.py), which the reference's post-3DGS trainer
 * (simple_trainer_worldmirror.py:776, :961) runs around every optimisation step.  Device fp32 / int32 buffers, no atomics, fixed order.
 * wm_densify_accumulate (every step; _update_state, default.py:220-260): for every Gaussian g, cameras c in order, where
 *   radii [C,N,2] has both entries > 0:  grad2d[g] += hypot(v_means2d[c,g,0] * width / 2 * C, v_means2d[c,g,1] * height / 2 * C),
 *   count[g] += 1, and, when radii_state is given, radii_state[g] = max(radii_state[g], max(rx, ry) / float(max(width, height)))
 *   (a true maximum over the cameras: the scatter-max default.py:255 names as intended; its indexed assignment keeps the last camera).
 *   v_means2d: the gradient or the absgrad of the backward above.  grad2d, count, radii_state [N] are updated in place.
 *   Asynchronous on stream, no workspace.
 * wm_densify_plan (at a refinement; _grow_gs + _prune_gs, default.py:263-339): with mean = grad2d / max(count, 1) and
 *   smax = max exp(scales [N,3]):  duplicate = mean > grow_grad2d and smax <= grow_scale3d;  split = (mean > grow_grad2d and
 *   smax > grow_scale3d) or (use_scale2d and radii_state > grow_scale2d).  grow_scale3d and prune_scale3d are passed already
 *   multiplied by the scene scale; use_scale2d = step < refine_scale2d_stop_iter (then radii_state is required);
 *   prune_big = step > reset_every.  Every entry that duplicate -> split would produce is then tested on ITS OWN values:
 *   pruned when sigmoid(opacity) < prune_opa, or, with prune_big, when its smax > prune_scale3d or (use_scale2d and its parent's
 *   radii_state > prune_scale2d); a split child has smax / 1.6 and, with revised_opacity, opacity 1 - sqrt(1 - sigmoid(o)).
 *   The survivors are laid out as ops.py:93-210 leaves them: un-split originals, duplicates, first split children, second split
 *   children, each in index order.  Per output row: src (source index), kind (0 keep, 1 duplicate, 2 / 3 first / second split
 *   child) and rank (for split rows: the parent's rank among ALL split Gaussians, pruned or not = its row of the noise); the three
 *   arrays have room for 3 N rows.  counts (HOST, 4 ints): n_dupli, n_split, n_prune, n_out, read back after ONE stream
 *   synchronisation (gsplat's .item()).  workspace: wm_densify_plan_workspace_bytes bytes.
 * wm_densify_gather: out [n_out,row] from in [N,row] by the plan.  mode 0 copy: every row = its source row (any parameter).
 *   1 zero_new: kind 0 rows copied, all others zero (Adam exp_avg / exp_avg_sq).  2 means (row 3): split children =
 *   mean + R(q / max(|q|, 1e-12)) (exp(s) * noise[b, rank]), b = 0 / 1 for kind 2 / 3, noise [2,N,3] standard normal draws
 *   supplied by the caller (rows [0, n_split) of each half are read), quats [N,4] wxyz, scales [N,3] log.  3 scales (row 3):
 *   split children = log(exp(s) / 1.6).  4 opacities_revised (row 1): split children = logit(1 - sqrt(1 - sigmoid(o))).
 *   quats / scales / noise are read in mode 2 only.  Asynchronous on stream, no workspace. */
wm_status wm_densify_accumulate(const float* v_means2d, const int* radii, int n_gaussians, int n_cameras, int width, int height,
                                float* grad2d, float* count, float* radii_state, void* stream);
size_t wm_densify_plan_workspace_bytes(size_t n_gaussians);
wm_status wm_densify_plan(const float* grad2d, const float* count, const float* radii_state, const float* scales, const float* opacities,
                          int n_gaussians, float grow_grad2d, float grow_scale3d, float grow_scale2d, float prune_opa, float prune_scale3d,
                          float prune_scale2d, int use_scale2d, int prune_big, int revised_opacity, int* src, int* kind, int* rank,
                          int* counts, void* workspace, size_t workspace_bytes, void* stream);
wm_status wm_densify_gather(const float* in, float* out, int n_gaussians, int row, int mode, const int* src, const int* kind,
                            const int* rank, int n_out, const float* quats, const float* scales, const float* noise, void* stream);

/* MCMC relocation, growth and position noise: gsplat's MCMCStrategy (gsplat/strategy/mcmc.py, ops.py:240-369; arXiv:2404.09591), the
 * other strategy of the reference's post-3DGS trainer.  Device fp32 / int32 buffers, log scales [N,3], logit opacities [N], quats [N,4]
 * wxyz; no float atomics, results independent of the launch order; asynchronous on stream except wm_mcmc_partition.
 * wm_mcmc_inject_noise (every step; inject_noise_to_position, ops.py:343-369): in place, for every Gaussian g
 *   means[g] += Sigma_g (noise[g] * gate_g * scaler),  Sigma = R diag(exp(s))^2 R^T,  R the rotation of q / max(|q|, 1e-12),
 *   gate = 1 / (1 + exp(-100 ((1 - sigmoid(o)) - 0.995))).  noise [N,3]: standard normal draws supplied by the caller.  No workspace.
 * wm_mcmc_partition (at a refinement; mcmc.py:154-155, ops.py:258-259): dead = sigmoid(o) <= min_opacity, or, when mask (one byte
 *   per Gaussian) is given, dead = mask != 0 and opacities is not read.  dead_idx and alive_idx (room for N ints each) receive the
 *   indices of the dead and of the other Gaussians, each in ascending order (as nonzero gives them).  counts (HOST, 2 ints):
 *   n_dead, n_alive, read back after ONE stream synchronisation (gsplat's .item()).  workspace: wm_mcmc_partition_workspace_bytes.
 * wm_mcmc_relocation (compute_relocation, relocation.py / RelocationCUDA.cu:26-43, with the ratios and the clamp of ops.py:272-278):
 *   for every j < n_sampled, g = sampled[j]:  ratio = clamp(number of entries of sampled equal to g, +1, 1, 51);  o = sigmoid(opacities[g]);
 *   x = 1 - (1 - o)^(1 / ratio);  denom = sum_{i=1..ratio} sum_{k=0..i-1} C(i-1, k) (-1)^k / sqrt(k+1) x^(k+1)  (paper eq. 9; evaluated
 *   in fp64 in its collapsed form sum_{k=0..ratio-1} C(ratio, k+1) (-1)^k / sqrt(k+1) x^(k+1), no table);
 *   new_scales[j] = log((o / denom) exp(scales[g]))  [n_sampled,3];  new_opacities[j] = logit(clamp(x, min_opacity, 1 - FLT_EPSILON))
 *   [n_sampled], clamped after the scale is computed.  hist: n_gaussians ints of scratch (zeroed here; integer atomics).
 * wm_mcmc_scatter (param_fn of relocate, ops.py:280-286, and of sample_add, ops.py:322-328): t [rows,row] in place; for every j
 *   v = values ? values[j] : t[sampled[j]];  t[sampled[j]] = v;  t[dest[j]] = v   (values [n_sampled,row] or null).
 *   dest holds distinct rows, none of which is in sampled.  sampled may repeat: every writer of a repeated row writes the same value
 *   (values of equal sources are equal by construction).  relocate: dest = the dead indices; sample_add: dest = N + j in a buffer of
 *   N + n rows whose first N rows the caller copied.  An index outside [0, rows) is skipped.
 * wm_mcmc_zero_rows (optimizer_fn of relocate, ops.py:288-290): t[idx[j]] = 0 for every j < n, t [rows,row]; idx may repeat. */
wm_status wm_mcmc_inject_noise(float* means, const float* quats, const float* scales, const float* opacities, const float* noise,
                               float scaler, int n_gaussians, void* stream);
size_t wm_mcmc_partition_workspace_bytes(size_t n_gaussians);
wm_status wm_mcmc_partition(const float* opacities, const unsigned char* mask, int n_gaussians, float min_opacity, int* dead_idx,
                            int* alive_idx, int* counts, void* workspace, size_t workspace_bytes, void* stream);
wm_status wm_mcmc_relocation(const float* opacities, const float* scales, const int* sampled, int n_sampled, int n_gaussians,
                             float min_opacity, float* new_opacities, float* new_scales, int* hist, void* stream);
wm_status wm_mcmc_scatter(float* t, int rows, int row, const int* sampled, const int* dest, const float* values, int n_sampled,
                          void* stream);
wm_status wm_mcmc_zero_rows(float* t, int rows, int row, const int* idx, int n, void* stream);

/* Fused L1 + SSIM photometric loss and its backward: the loss of the reference's "Post 3DGS Optimization" (README; gsplat's
 * simple_trainer_worldmirror.py:785-792: F.l1_loss(colors, pixels) and 1 - fused_ssim(colors, pixels, padding="valid"), mixed with
 * ssim_lambda = 0.2 by the caller).  fused_ssim is a CUDA-only extension; this is the published definition it implements:
 *   window: 1-D Gaussian of 11 taps, sigma 1.5, normalised to sum 1; the 2-D window G is its outer product; all five filters
 *   below are depthwise with zero padding 5.  For a = img1 (the render), b = img2 (the target):
 *   mu1 = G*a, mu2 = G*b, s1 = G*(a a) - mu1^2, s2 = G*(b b) - mu2^2, s12 = G*(a b) - mu1 mu2, C1 = 0.01^2, C2 = 0.03^2,
 *   map = (2 mu1 mu2 + C1)(2 s12 + C2) / ((mu1^2 + mu2^2 + C1)(s1 + s2 + C2)).
 *   *out_ssim = mean of map over B C H W (padding_valid = 0, "same") or over the map cropped by 5 on every side, B C (H-10) (W-10)
 *   elements (padding_valid = 1); *out_l1 = mean |a - b| over B C H W.
 * img1 / img2: fp32 [B,C,H,W] addressed by ELEMENT strides strides1 / strides2 = (sB, sC, sH, sW) (host arrays, read during the
 * call): contiguous NCHW and the permuted view of a channels-last [B,H,W,C] tensor are both read in place.  out_ssim, out_l1:
 * device floats.  want_backward = 1 also leaves d map / d mu1, d map / d s1 and d map / d s12 (zero outside the counted region) in
 * the workspace for the backward call; want_backward = 0 gives the same two values, bit for bit.
 * Backward: grad_img1 (fp32, img1's strides, overwritten) = *g_ssim * d ssim / d img1 + *g_l1 * sign(a - b) / (B C H W), sign(0) = 0;
 * g_ssim, g_l1: device floats.  img2 gets no gradient.  CONTRACT: the same images, sizes, padding_valid and workspace as the
 * forward call with want_backward = 1, the workspace UNTOUCHED in between.
 * workspace: wm_photometric_loss_workspace_bytes bytes (12 bytes per image element + 16 per 32 x 32 tile) for the forward with
 * want_backward = 1 and for the backward; a forward with want_backward = 0 touches the per-tile part only and accepts a workspace
 * of wm_photometric_loss_forward_workspace_bytes bytes.
 * Both calls are asynchronous on stream and never synchronise the host.  Sums run in a fixed order, no atomics: results are bitwise
 * reproducible, and identical between layouts of the same values.  WM_ERR_INVALID: a size <= 0, padding_valid with H < 11 or
 * W < 11 (the mean of an empty map), a workspace that is too small, a null pointer. */
size_t wm_photometric_loss_workspace_bytes(int B, int C, int H, int W);
size_t wm_photometric_loss_forward_workspace_bytes(int B, int C, int H, int W);
wm_status wm_photometric_loss(const float* img1, const int64_t* strides1, const float* img2, const int64_t* strides2, int B, int C,
                              int H, int W, int padding_valid, int want_backward, float* out_ssim, float* out_l1,
                              void* workspace, size_t workspace_bytes, void* stream);
wm_status wm_photometric_loss_backward(const float* img1, const int64_t* strides1, const float* img2, const int64_t* strides2, int B,
                                       int C, int H, int W, int padding_valid, const float* g_ssim, const float* g_l1,
                                       float* grad_img1, const void* workspace, size_t workspace_bytes, void* stream);

/* Bilateral-grid appearance correction of the post-3DGS trainer (gsplat's simple_trainer_worldmirror.py:812-814 under
 * --use_bilateral_grid, :555-570 for the loss term).  The trainer's --use_fused_bilagrid package is CUDA-only; these entries are
 * the semantics of its pure-torch twin, examples/lib_bilagrid.py.
 * slice (lib_bilagrid.py:180-244 with BilateralGrid.forward :310-365 and color_affine_transform :141-154):
 *   grids fp32 [G,12,L,Hg,Wg], channel 4 r + c = entry (r, c) of a 3 x 4 matrix; grid_idx int32 [B] ON THE DEVICE; xy [B,n,2] in
 *   [0,1], rgb [B,n,3], out [B,n,3], all contiguous fp32.  Sample j of row b reads grid grid_idx[b] at
 *   (2 (x - .5), 2 (y - .5), 2 (.299 r + .587 g + .114 b) - 1) as F.grid_sample(mode="bilinear", align_corners=True,
 *   padding_mode="border") does: u = (c + 1) / 2 * (size - 1) clamped to [0, size - 1], trilinear; the 12 numbers A give
 *   out = A[:, :3] rgb + A[:, 3].  The [.., 3, 4] matrices ("rgb_affine_mats") are never written anywhere.
 *   A row whose index is outside [0, G) reads no grid: its out (and its v_rgb) are NaN and it adds nothing to v_grids.
 * backward: v_out [B,n,3].  v_grids [G,12,L,Hg,Wg]: EVERY element is written (zeros for a grid that no row names; rows naming one
 *   grid sum); v_rgb [B,n,3] = A[:, :3]^T v_out + the term through the guidance coordinate, which is zero where that coordinate
 *   sits on or outside the clamp range (torch's rule).  Either of v_grids, v_rgb may be NULL: that gradient is not computed.  xy gets none.
 *   The workspace (needed for v_grids only) holds one partial grid gradient per block: 48 L Hg Wg bytes times at most 256 blocks
 *   (B rows x segments per row).  Sums run in a fixed order (sample, row, segment), no atomics: identical bits run to run.
 * total variation (lib_bilagrid.py:161-177) of x fp32 [B,C,L,H,W], contiguous: the sum over the three trailing axes of
 *   sum (x shifted by one - x)^2 / max(C L H W with that axis one shorter, 1), divided by B -> *out (device float).
 *   Backward: v_x (same shape, every element written) = *g (device float) * d tv / d x.  The workspace of the value call holds one
 *   double per block (at most 8 KiB).
 * LIMITS: L * Hg * Wg <= 4096 cells and each of L, Hg, Wg <= 1024 (the grid gradient keeps a block's cells in registers; the
 *   default 16 x 16 x 8 is 2048); B * n < 2^29.  Larger shapes are refused by all three slice entries, there is no slower path.
 * Every call is asynchronous on stream and never synchronises the host.  WM_ERR_INVALID, before anything is launched: a size <= 0,
 * a shape beyond the limits, a null pointer where none is allowed, a workspace that is too small. */
wm_status wm_bilagrid_slice(const float* grids, int G, int L, int Hg, int Wg, const int* grid_idx, const float* xy, const float* rgb,
                            int B, int n, float* out, void* stream);
size_t wm_bilagrid_slice_backward_workspace_bytes(int G, int L, int Hg, int Wg, int B, int n);
wm_status wm_bilagrid_slice_backward(const float* grids, int G, int L, int Hg, int Wg, const int* grid_idx, const float* xy,
                                     const float* rgb, int B, int n, const float* v_out, float* v_grids, float* v_rgb,
                                     void* workspace, size_t workspace_bytes, void* stream);
size_t wm_bilagrid_tv_workspace_bytes(int B, int C, int L, int H, int W);
wm_status wm_bilagrid_tv(const float* x, int B, int C, int L, int H, int W, float* out, void* workspace, size_t workspace_bytes,
                         void* stream);
wm_status wm_bilagrid_tv_backward(const float* x, int B, int C, int L, int H, int W, const float* g, float* v_x, void* stream);

/* Appearance optimisation of the post-3DGS trainer — replaces gsplat's AppearanceOptModule (examples/utils.py:51-114), which
 * simple_trainer_worldmirror.py builds under --app_opt (:532-552) and evaluates per step (:603-611): per (camera c, Gaussian g) pair
 *   h = [embeds[embed_ids[c]] (16) | features[g] (32) | B_k(dirs[c,g] / max(|dirs[c,g]|, 1e-12)), k < (module_sh_degree + 1)^2],
 *   out[c,g,:] = W3 relu(W2 relu(W1 h + b1) + b2) + b3, with B_k = 0 for k >= (sh_degree + 1)^2 (bands the call does not use); pre-sigmoid.
 * B_k: the real SH basis of raster_sh / gsplat's _eval_sh_bases_fast.  Built for feature_dim 32, embed_dim 16, mlp_width 64, mlp_depth 2:
 * W1 [64, 48 + (module_sh_degree + 1)^2] (columns in the module's order: embedding, features, basis), b1 [64], W2 [64,64], b2 [64], W3 [3,64],
 * b3 [3]; embeds [n_embeds,16]; embed_ids int32 [C] ON THE DEVICE or null (zero embeddings; an id outside [0, n_embeds) also reads zeros
 * and receives no gradient); features [N,32], dirs [C,N,3], out [C,N,3]; all contiguous fp32.  0 <= sh_degree <= module_sh_degree <= 3.
 * All arithmetic is fp32 (the matrix products on the exact fp32-input MFMA); nothing of size [C,N,64] is written.
 * backward (examples/utils.py:51-114 differentiated): v_out [C,N,3] -> v_features [N,32] (summed over the cameras in camera order by one
 *   writer), v_dirs [C,N,3] (through the basis and the normalisation; finite for a zero direction), v_W1 .. v_b3 in the shapes above (basis
 *   columns of bands the call does not use: exact zeros), v_embeds [n_embeds,16] (optional; every element written, rows no camera names
 *   are zeros, a repeated id sums in camera order).  ReLU's gradient is taken where the pre-activation is > 0.  The activations are
 *   recomputed, none is stored.  The weight gradients are summed without atomics: a grid of min(ceil(N / 128), 512) blocks, each over a
 *   contiguous run of 128-Gaussian tiles, leaves one partial set per block in the workspace and a second kernel adds them in block order:
 *   identical bits run to run.  workspace: wm_appearance_backward_workspace_bytes bytes (about 30 KB + 1 KB per camera, per block); a
 *   smaller one returns WM_ERR_INVALID before anything is launched.
 * Both calls are asynchronous on stream and never synchronise the host.  WM_ERR_INVALID, before anything is launched: a size <= 0, a degree
 * outside the ranges above, N * C >= 2^29, a null pointer where none is allowed. */
wm_status wm_appearance_forward(const float* features, const float* embeds, int n_embeds, const int* embed_ids, const float* dirs,
                                const float* W1, const float* b1, const float* W2, const float* b2, const float* W3, const float* b3,
                                int n_gaussians, int n_cameras, int module_sh_degree, int sh_degree, float* out, void* stream);
size_t wm_appearance_backward_workspace_bytes(int n_gaussians, int n_cameras);
wm_status wm_appearance_backward(const float* features, const float* embeds, int n_embeds, const int* embed_ids, const float* dirs,
                                 const float* W1, const float* b1, const float* W2, const float* b2, const float* W3, const float* b3,
                                 int n_gaussians, int n_cameras, int module_sh_degree, int sh_degree, const float* v_out,
                                 float* v_features, float* v_dirs, float* v_embeds, float* v_W1, float* v_b1, float* v_W2, float* v_b2,
                                 float* v_W3, float* v_b3, void* workspace, size_t workspace_bytes, void* stream);

/* Depth supervision of the post-3DGS trainer: the sparse disparity loss of gsplat's simple_trainer_worldmirror.py:793-811 (the
 * `if cfg.depth_loss:` block: normalise the pixel coordinates with (width - 1, height - 1), F.grid_sample(align_corners=True), disparity,
 * F.l1_loss against 1 / depths_gt; scene_scale and depth_lambda stay with the caller), and the projection that produces its points,
 * examples/datasets/colmap.py:412-433 (the `if self.load_depths:` block of Dataset.__getitem__).
 * loss.  depth: fp32 [C,H,W] addressed by ELEMENT strides (sC, sH, sW) (host array, read during the call): channel 3 of a [C,H,W,4]
 *   render is read in place.  points [C,M,2] (x, y) in pixels with pixel centres at integers, depth_gt [C,M], contiguous fp32; valid [C,M]
 *   bytes, 0 = the row does not exist (its coordinates and its depth_gt are never read and may be NaN), or NULL = every row counts.
 *   Row (c, m) reads camera c's image at x0 = floor(x), y0 = floor(y), fx = x - x0, fy = y - y0:
 *     d = (1-fx)(1-fy) D[y0,x0] + fx (1-fy) D[y0,x0+1] + (1-fx) fy D[y0+1,x0] + fx fy D[y0+1,x0+1], a corner outside the image counting as 0
 *     (zero padding: x in (W - 1, W) and y in (H - 1, H), which the projection keeps, lose their right / lower corners; a point
 *     further out than one pixel samples 0);  disp = d > 0 ? 1 / d : 0;  term = |disp - 1 / depth_gt|.
 *   *out_loss (device float) = sum of the terms / n, n = the number of valid rows, both found on the device in the same pass; the sum
 *   runs in fp64 in a fixed order and is rounded once.  n = 0 (M = 0 included) gives NaN, as torch's mean of an empty tensor.
 * backward.  v_depth (fp32, EVERY element written, addressed by the element strides v_strides = (sC, sH, sW), a host array: pass the depth
 *   image's own strides to write a gradient laid out as the image is) =
 *     v_depth[c,y,x] = (*g / n) * sum_m w_m(y,x) * sign(disp_m - 1 / depth_gt_m) * (-1 / d_m^2)
 *   over the valid rows of camera c whose four corners hold (y, x), w_m the corner's bilinear weight; sign(0) = 0 and a row with
 *   d_m <= 0 adds nothing; n = 0 gives zeros.  g: device float.  points and depth_gt get no gradient.  A pixel's sum runs in row order
 *   (a stable sort by cell, then a merge by row index), without floating-point atomics: identical bits run to run and between two
 *   layouts of the same depth values.  A cell's rows are walked by one lane, so a call's time grows with the largest number of rows in
 *   one cell (all M rows of a camera in one cell: O(M) steps of one lane).  CONTRACT: the same sizes, points and workspace as the forward
 *   call with want_backward = 1, the workspace UNTOUCHED in between: that call leaves n and one coefficient per row there, so the
 *   backward reads neither the depth image nor depth_gt nor valid again and does not take them.
 * workspace: wm_depth_loss_workspace_bytes(C, H, W, M, want_backward) bytes: want_backward = 0: 16 bytes per 256 rows; 1: about 20 bytes
 *   per row + 4 per pixel + the sort's scratch, counted as 8 bytes per row + 1 MiB (a rule of this library, the same number on every
 *   machine; the backward returns WM_ERR_HIP should the sort ever ask for more).  0 for sizes the calls refuse.
 * wm_project_depth_points.  points_world [P,3], camtoworlds [C,4,4], Ks [C,3,3] contiguous fp32; visible [C,P] bytes or NULL (stands
 *   for the reference's per-image point_indices) -> points [C,P,2], depths [C,P] fp32, valid [C,P] bytes.  p_cam = R^T (p_world - t) with
 *   [R | t] the top three rows of camtoworld: the RIGID inverse, taken inside the call per camera in fp64 (R is assumed orthonormal; the
 *   reference inverts the 4 x 4); q = K p_cam, (x, y) = q.xy / q.z, depth = p_cam.z, all in fp64 with one rounding per output;
 *   valid = visible && 0 <= x < width && 0 <= y < height && depth > 0, tested on the fp64 values.  Nothing is compacted: the loss takes
 *   valid, so cameras with different numbers of points need no ragged layout.
 * All calls are asynchronous on stream and never synchronise the host.  WM_ERR_INVALID, before anything is launched: a null pointer where
 * none is allowed, C < 1, H < 2 or W < 2 (the reference's normalisation divides by W - 1 and H - 1; the projection accepts 1), M < 0 or
 * P < 0, C (H + 1) (W + 1) >= 2^31 - 1, C M >= 2^30, a workspace that is too small.  M = 0 is legal: the n = 0 case. */
size_t wm_depth_loss_workspace_bytes(int C, int H, int W, int M, int want_backward);
wm_status wm_depth_loss(const float* depth, const int64_t* strides, int C, int H, int W, const float* points, const float* depth_gt,
                        const unsigned char* valid, int M, int want_backward, float* out_loss, void* workspace, size_t workspace_bytes,
                        void* stream);
wm_status wm_depth_loss_backward(int C, int H, int W, const float* points, int M, const float* g, float* v_depth,
                                 const int64_t* v_strides, void* workspace, size_t workspace_bytes, void* stream);
wm_status wm_project_depth_points(const float* points_world, const float* camtoworlds, const float* Ks, const unsigned char* visible,
                                  int C, int P, int width, int height, float* points, float* depths, unsigned char* valid, void* stream);

/* ---- Splat export (csrc/export.hip): the file bodies of gsplat's export_splats, gsplat/exporter.py:475-553 with :363-417 ("ply"),
 * :420-472 ("splat"), :194-360 ("ply_compressed") and the Morton order of :56-85, and of the hand-off file of
 * src/utils/save_utils.py:133-188 (save_gs_ply).  The body is produced on the device in the byte order of the file; the caller writes the
 * text header and copies the body to the host once.
 * inputs.  means [N,3], scales [N,3] (log), quats [N,4], opacities [N] (logit), sh0 [N,3], shN [N,K,3] (K = 0: may be NULL), contiguous fp32
 *   on the device.  K <= 15 (degree 3).
 * keep.  A row is kept when all of its 14 + 3K numbers are finite and, for WM_EXPORT_PLY_COMPRESSED, 1 / (1 + exp(-opacity)) >
 *   opacity_threshold (the reference's default is 1 / 255).  Kept rows stay in input order.  *n_kept (host) is written before the call
 *   returns: the call synchronises the stream ONCE, to read that count, and launches the packing kernels behind it; the body itself is
 *   complete in stream order.  It occupies the first payload_bytes(*n_kept, K, format) bytes of out.
 * WM_EXPORT_PLY.  fp32 rows [x y z | f_dc_0..2 | f_rest_0..3K-1 | opacity | scale_0..2 | rot_0..3], f_rest channel-major (column c K + k is
 *   shN[i, k, c]), the parameters as given.
 * WM_EXPORT_SPLAT.  32-byte records in Morton order: 3 x f32 mean, 3 x f32 exp(scale), 4 x u8 trunc(clamp(255 [0.5 + C0 sh0,
 *   sigmoid(opacity)], 0, 255)), 4 x u8 trunc(clamp(q / |q| 128 + 128, 0, 255)).
 * WM_EXPORT_PLY_COMPRESSED.  [18 floats per chunk of 256 splats of the Morton order | 4 x u32 per splat | 3K bytes per splat]: the chunk's
 *   min / max of the means, of the log-scales (clamped to +-20) and of 0.5 + C0 sh0; position 11-10-11, rotation 2 + 3 x 10, scale 11-10-11,
 *   colour and sigmoid(opacity) 8-8-8-8, each field clamp(floor(v (2^b - 1) + 0.5), 0, 2^b - 1); sh bytes trunc(clamp((x / 8 + 0.5) 256, 0, 255)).
 * Morton order.  floor((c - min) / len * 1024) per axis over the kept means (len = 0 -> 1), low 10 bits, interleaved z y x; a stable sort,
 *   so equal codes stay in input order.
 * All arithmetic is fp32 in the reference's operation order without fused multiply-adds; the results are bitwise reproducible.
 * Defined here where the reference is not: a chunk quantity with max == min packs as field 0; no kept row gives *n_kept = 0 and an empty
 *   body; a non-finite opacity drops that row alone (the reference drops every row).
 * workspace: the _workspace_bytes value for (N, K, format): 12 bytes per row, for the two Morton formats 16 more per row + 24 per 256 rows,
 *   and the library scan's / sort's scratch counted as 8 bytes per row + 1 MiB (a rule of this library, the same number on every machine;
 *   WM_ERR_HIP should the library ever ask for more).  out_bytes >= the _payload_bytes value for (N, K, format), the size if every row is kept.
 *   Both size calls return 0 for arguments the export refuses.
 * WM_ERR_INVALID, before anything is launched: a null pointer where none is allowed (N = 0 allows null tensors and a null out), N < 0,
 *   N >= 2^31, K < 0, K > 15, an unknown format, a workspace or an output buffer that is too small. */
typedef enum { WM_EXPORT_PLY = 0, WM_EXPORT_SPLAT = 1, WM_EXPORT_PLY_COMPRESSED = 2 } wm_export_format;
size_t wm_export_splats_workspace_bytes(int64_t N, int K, int format);
size_t wm_export_splats_payload_bytes(int64_t n_kept, int K, int format);
wm_status wm_export_splats(const float* means, const float* scales, const float* quats, const float* opacities, const float* sh0,
                           const float* shN, int64_t N, int K, int format, float opacity_threshold, void* workspace, size_t workspace_bytes,
                           void* out, size_t out_bytes, int* n_kept, void* stream);
/* The row packer behind WM_EXPORT_PLY, for any column list (src/utils/save_utils.py:154-185: the masked gathers, the zero normals,
 * scales.log() and the concatenation of save_gs_ply).  out [n_kept, n_cols] fp32: out[r, c] = f_c(col_ptrs[c][i_r * col_strides[c]]) for
 * the r-th row i_r with keep[i_r] != 0 (keep: N bytes on the device, NULL = every row), f_c = identity (WM_PACK_NONE) or log
 * (WM_PACK_LOG, the library's logf); col_ptrs[c] = NULL is a column of zeros.  col_ptrs, col_strides (in elements) and col_transforms are
 * host arrays of n_cols entries, 1 <= n_cols <= 64; the pointers in col_ptrs are device pointers.  *n_kept and the one stream
 * synchronisation as above.  workspace: the _workspace_bytes value for N (12 bytes per row + the scan's scratch as above);
 * out_bytes >= N * n_cols * 4.  WM_ERR_INVALID, before anything is launched: a null array, n_cols outside 1..64, a negative stride, an
 * unknown transform, N < 0, N >= 2^31, a null or too small workspace, a too small or (N > 0) null out. */
typedef enum { WM_PACK_NONE = 0, WM_PACK_LOG = 1 } wm_pack_transform;
size_t wm_pack_rows_workspace_bytes(int64_t N);
wm_status wm_pack_rows(const float* const* col_ptrs, const int* col_strides, const int* col_transforms, int n_cols,
                       const unsigned char* keep, int64_t N, void* workspace, size_t workspace_bytes, float* out, size_t out_bytes,
                       int* n_kept, void* stream);

/* ---- COLMAP hand-off (csrc/colmap.hip): the sparse model the post-3DGS trainer starts from, infer.py:269-358 with
 * src/utils/build_pycolmap_recon.py, and the coloured point clouds of src/utils/save_utils.py:81-130.
 * selection (infer.py:296-335).  depth, conf [S,H,W] and images [S,3,H,W] contiguous fp32 on the device, camtoworlds [S,4,4] (the inverse
 *   of the stored world-to-camera pose) and intrinsics [S,3,3] at H x W.  A pixel is a candidate when depth > eps (the mask of
 *   wm_depth_to_world); the candidates are ordered view-major, row-major inside a view.  Of the N_valid candidates the
 *   K = max(1, ceil(N_valid (100 - p) / 100)) highest confidences are kept (p <= 0: all; the arithmetic in double), conf <= 1e-5 counting
 *   as -inf and ties at the K-th value going to the lowest candidate index (the rules of wm_confidence_mask).  The kept candidates keep their
 *   order: positions come from prefix sums, never from atomics, and do not depend on block scheduling.
 *   The select entry leaves its state in the workspace, synchronises the stream ONCE and writes *n_kept and counts[S] (host: kept points in all
 *   and per view; N_valid = 0 gives zeros).  The gather entry, given the same arguments and the untouched workspace, writes points [n_kept,3]
 *   fp32 (the expressions of wm_depth_to_world), colors [n_kept,3] u8 = trunc(clamp(image, 0, 1) 255) (the reference does not clamp; NaN
 *   gives 0) and xyf [n_kept,3] int32 = (trunc(x scale_x), trunc(y scale_y), view), the products in double as numpy takes them.
 *   workspace: the _workspace_bytes value for (S, H, W): about 12 bytes per 512 pixels; 0 for S, H or W < 1 or S H W >= 2^31.
 * packing (build_pycolmap_recon.py:36-51, 76-77 and the per-point part of pycolmap's write).  points [P,3] fp32, colors [P,3] u8, xyf [P,3]
 *   int32, counts [S] int64 on the device, the points view-major with counts[i] of view i.  points3d receives 59 bytes per point: u64 id =
 *   index + 1, 3 x f64 xyz, 3 x u8 rgb, f64 error = -1, u64 track length = 1, u32 image_id = view + 1, u32 point2D_idx = index - (points
 *   of earlier views).  points2d receives 24 bytes per point: f64 x, f64 y, u64 point3D_id.  Little-endian, no padding; either buffer may
 *   be NULL.  points3d must be 4-byte and points2d 8-byte aligned.  The caller owns the headers and the per-image headers that go between
 *   the views' runs of points2d.  No synchronisation.  workspace: the _workspace_bytes value for (P, S); 0 for P < 0, P >= 2^31, S < 1.
 * point-cloud PLY rows (save_utils.py:86-111, 119-127): 15 bytes per kept row, 3 x f32 xyz and 3 x u8 rgb, of the rows with keep[i] != 0
 *   (keep: N bytes on the device), or, with keep NULL and filter_finite != 0, of the rows whose three coordinates are finite, or of every
 *   row; input order.  *n_kept (host) is written before the call returns; the call synchronises once when it filters and not otherwise.
 *   out: 4-byte aligned, out_bytes >= 15 N.  workspace: the _workspace_bytes value for N (about 4 bytes per row); 0 for N < 0, N >= 2^31.
 * WM_ERR_INVALID, before anything is launched: a null pointer where none is allowed, sizes the size calls refuse, a too small workspace or
 *   output buffer, a misaligned output. */
size_t wm_colmap_select_workspace_bytes(int S, int H, int W);
wm_status wm_colmap_select(const float* depth, const float* conf, int S, int H, int W, float eps, double conf_threshold_percent,
                           void* workspace, size_t workspace_bytes, int64_t* n_kept, int64_t* counts, void* stream);
wm_status wm_colmap_gather(const float* depth, const float* conf, const float* images, const float* camtoworlds, const float* intrinsics,
                           int S, int H, int W, float eps, double scale_x, double scale_y, const void* workspace, size_t workspace_bytes,
                           int64_t n_kept, float* points, unsigned char* colors, int32_t* xyf, void* stream);
size_t wm_colmap_pack_workspace_bytes(int64_t P, int S);
wm_status wm_colmap_pack(const float* points, const unsigned char* colors, const int32_t* xyf, const int64_t* counts, int S, int64_t P,
                         void* workspace, size_t workspace_bytes, void* points3d, size_t points3d_bytes, void* points2d,
                         size_t points2d_bytes, void* stream);
size_t wm_pack_point_ply_workspace_bytes(int64_t N);
wm_status wm_pack_point_ply(const float* points, const unsigned char* colors, const unsigned char* keep, int filter_finite, int64_t N,
                            void* workspace, size_t workspace_bytes, void* out, size_t out_bytes, int64_t* n_kept, void* stream);

/* ---- k nearest neighbours of a cloud within itself (csrc/knn.hip): the reference's knn, submodules/gsplat/examples/utils.py:141-145 (a copy
 * to the host and scikit-learn's kd-tree), as the trainer's splat initialisation calls it, simple_trainer_worldmirror.py:334-337
 * (scales = log(sqrt(mean(knn(points, 4)[:, 1:]^2)) init_scale)).
 * points [N,3] contiguous fp32 on the device.  dist [N,K] fp32: row i holds the K smallest values of |x_i - x_j| over ALL j, ascending, the
 * point itself included (column 0 is 0, as scikit-learn's kneighbors(X) on the fitted set), each computed in fp32 in difference form,
 * sqrt(dx dx + dy dy + dz dz) with dx = x_i - x_j and no fused multiply-add; duplicates give exact zeros.  idx [N,K] int32 (may be NULL): the
 * rows j, ties ordered by row (a tie at the K-th place, or a row full of zeros, may keep any of the tied rows).  Rows are in input order.
 * Exact: the Morton-sorted cell structure only prunes, and every comparison that ends a search is conservative in fp32.  The same input
 * gives the same bits.  *nonfinite_flag (one int on the device, written by the call): 0, or 1 when a coordinate is NaN or infinite, and
 * then dist and idx are not written; the caller reads it (the only synchronisation the operation needs).  The call itself does not
 * synchronise and runs no host loop that depends on the data.
 * Worst case: a pass of a query costs the points of its 3 x 3 x 3 cells.  A dense part smaller than 2^-21 of the bounding box is one cell
 * and is scanned by each of its queries; a far outlier scans up to the whole cloud.  Both stay exact.
 * workspace: the _workspace_bytes value for (N, K): 44 bytes per point + the sort's scratch; 0 for sizes the call refuses.
 * WM_ERR_INVALID, before anything is launched: K < 1, K > 16, K > N, N >= 2^31, a null pointer other than idx, a too small workspace. */
size_t wm_knn_workspace_bytes(int64_t N, int K);
wm_status wm_knn(const float* points, int64_t N, int K, void* workspace, size_t workspace_bytes, float* dist, int32_t* idx,
                 int32_t* nonfinite_flag, void* stream);

/* ---- the nearest point of ANOTHER cloud (csrc/knn.hip), the search under a point-cloud evaluation (accuracy / completeness, ICP): an index
 * built once over ref [N,3] and queried many times.  The reference ships no evaluation code; the semantics are this library's own.
 * build: ref [N,3] contiguous fp32 on the device; index: index_bytes >= the wm_nearest_build_workspace_bytes value for N (40 bytes per point + the sort's
 *   scratch), the caller's memory, opaque, valid for this N until it is overwritten.  *nonfinite_flag (one int on the device, written by
 *   the call): 0, or 1 when a coordinate of ref is NaN or infinite; such an index answers no query (a query call then writes nothing).
 * query: queries [M,3] contiguous fp32 on the device, anywhere in space.  dist [M] fp32: dist[i] = the minimum over ALL j of
 *   sqrt(dx dx + dy dy + dz dz), dx = q_i.x - r_j.x, in fp32, every operation rounded on its own (no fused multiply-add), the distance rule of
 *   wm_knn.  idx [M] int32 (may be NULL): the lowest row j that attains the minimum of the squared fp32 value.  A query row with a NaN or
 *   infinite coordinate gets dist = NaN and idx = -1; the other rows are unaffected.  Rows are in input order.  M = 0 launches nothing.
 * Exact: the Morton-sorted cell structure only prunes, and every pruning comparison is conservative in fp32 for a query at any distance
 * from the box (csrc/knn.hip).  The same input gives the same bits.  Neither call synchronises or runs a host loop that depends on the data.
 * Worst case: a query costs the points of the cells its best-distance ball touches.  All of ref inside one finest cell (2^-21 of the
 * extent) is scanned by every query; a query farther away than 10^4 extents sees the whole cloud at one distance and scans it.  Exact both.
 * workspace of a query: the _workspace_bytes value for M (24 bytes per query + the sort's scratch).
 * WM_ERR_INVALID, before anything is launched: N < 1, N or M >= 2^31, M < 0, a null pointer other than idx (with M = 0: other than idx,
 *   queries and dist), index_bytes or workspace_bytes too small. */
size_t wm_nearest_build_workspace_bytes(int64_t N);
wm_status wm_nearest_build(const float* ref, int64_t N, void* index, size_t index_bytes, int32_t* nonfinite_flag, void* stream);
size_t wm_nearest_query_workspace_bytes(int64_t M);
wm_status wm_nearest_query(const void* index, size_t index_bytes, int64_t N, const float* queries, int64_t M, void* workspace,
                           size_t workspace_bytes, float* dist, int32_t* idx, void* stream);

/* ---- the reductions of a point-cloud evaluation (csrc/reconmetrics.hip).  Every sum is fp64 in a fixed order that depends on the element
 * count alone (a two-level sum: threads, then blocks): the same input gives the same bits.  No call synchronises.
 * wm_cloud_stats: one direction of accuracy / completeness over a result of wm_nearest_query.  dist [M] fp32, idx [M] int32 (read only with
 *   normals).  out (device, 4 + WM_STATS_MAX_THRESHOLDS doubles): [0] the mean of dist; [1] its median with numpy's rule (the exact order
 *   statistics of rank floor((M - 1) / 2) and floor(M / 2) by radix selection, their mean in fp64); [2], [3] with normals_a [M,3] and
 *   normals_b [Nb,3] the mean and median of |n_a[i] . n_b[idx[i]]|, the product in fp32 with every operation rounded on its own, NaN where idx[i]
 *   is outside 0 .. Nb-1, and left unwritten without normals; [4 + k] the count of dist < thresholds[k], k < n_thresholds <=
 *   WM_STATS_MAX_THRESHOLDS (thresholds: a HOST array, read before the call returns).  A NaN makes the mean NaN and ranks above +inf.
 * wm_umeyama: the similarity (s, R, t) that minimises the sum of |dst_i - (s R src_i + t)|^2 over the pairs with mask[i] != 0 (mask [P]
 *   bytes on the device, or NULL for all): Umeyama's closed form (IEEE TPAMI 13(4), 1991).  src, dst [P,3] fp32.  The count and the two
 *   means in one pass, the centred cross-covariance and the source variance in a second, the 3 x 3 singular value decomposition by one-sided
 *   Jacobi rotations on one thread, the last singular direction mirrored when det U det V < 0 so that R is a rotation.  out (device, 16
 *   doubles): s (1 with with_scale = 0), R [9] row-major, t [3], the count, the source variance, 0.  Fewer than 3 pairs, or collinear ones,
 *   leave R undetermined (a count of 0 gives NaNs); the caller reads the count.
 * workspace: the _workspace_bytes values; 0 for sizes the calls refuse.
 * WM_ERR_INVALID, before anything is launched: M or P < 1 or >= 2^31, n_thresholds outside 0 .. WM_STATS_MAX_THRESHOLDS, a null pointer
 *   where none is allowed (idx and normals_b with normals_a, thresholds with n_thresholds > 0), Nb < 1 with normals, a too small workspace. */
#define WM_STATS_MAX_THRESHOLDS 16
size_t wm_cloud_stats_workspace_bytes(int64_t M);
wm_status wm_cloud_stats(const float* dist, const int32_t* idx, int64_t M, const float* normals_a, const float* normals_b, int64_t Nb,
                         const float* thresholds, int n_thresholds, void* workspace, size_t workspace_bytes, double* out, void* stream);
size_t wm_umeyama_workspace_bytes(int64_t P);
wm_status wm_umeyama(const float* src, const float* dst, const unsigned char* mask, int64_t P, int with_scale, void* workspace,
                     size_t workspace_bytes, double* out, void* stream);

/* ---- fly-through video around the rasteriser (csrc/video.hip): what src/utils/render_utils.py:196-368 render_interpolated_video runs per frame
 * beside rasterize_batches.
 *
 * wm_gs_effect_spread: GSEffects.apply_effect with effect_type 2 (src/utils/gs_effects.py:162-242) in one pass, with the driver's composition
 * of render_utils.py:230-234 folded in.  means / scales / colors [N,3], opacities / random_vals [N], all contiguous fp32 on the device.
 * Positions enter as (means - shift) * inv_scale and scales as scales * inv_scale (shift: 3 floats ON THE DEVICE, or NULL for none; inv_scale 1
 * for none); colors_are_sh0 != 0: colors are degree-0 SH, converted by sh * C0 + 0.5 on the way in and (rgb - 0.5) / C0 on the way out
 * (C0 = 0.28209479177387814).  t_n is the reference's normalized_t = t - start_time; its host scalars (s = smoothstep of t_n - 3.2 times 10,
 * t_n - 3.1416) are taken in fp64 as Python takes them and then used in fp32 as the tensor operations use them.  Outputs: out_means,
 * out_scales, out_colors [N,3], out_opacities [N] and flag [N] = the reference's smoothstep_val; with ignore_scale the scale mix and the
 * random mask (random_vals < 0.8 flag, which zeroes means, scales and opacities) are skipped.  The noise term of gs_effects.py:211-218 is not
 * evaluated: the reference multiplies it by 0.0, so it shows only for non-finite positions, which are out of contract.
 * stats (device, 2 doubles, written by the call): [0] the number of flag < 0.99 (render_utils.py:228), [1] the sum of flag in fp64
 * (render_utils.py:281 takes its mean), both by a fixed-order two-stage reduction: the same input gives the same bits.  No synchronisation.
 * Not built: the trainer-parametrised output of render_utils.py:236-241 (log scales, logit opacities).
 * WM_ERR_INVALID, before anything is launched: N < 0, N >= 2^31, a NaN t_n, a null pointer other than shift, a too small workspace. */
size_t wm_gs_effect_spread_workspace_bytes(int64_t N);
wm_status wm_gs_effect_spread(const float* means, const float* scales, const float* opacities, const float* colors, const float* random_vals,
                              int64_t N, double t_n, int ignore_scale, const float* shift, float inv_scale, int colors_are_sh0, float* out_means,
                              float* out_scales, float* out_opacities, float* out_colors, float* flag, double* stats, void* workspace,
                              size_t workspace_bytes, void* stream);
/* wm_video_frames: the frames in bytes.  rgbs [F,H,W,3] fp32 (or NULL) -> rgb_out [F,H,W,3] u8 = uint8 of clamp to [0, 1] times 255, the fp32
 * product truncated (_make_video, render_utils.py:355-357).  depths [F,H,W] fp32 (or NULL) -> depth_out [F,H,W,3] u8 and near_far [F,2] fp32:
 * depth_vis of render_utils.py:326-335 per frame, near = log of torch.quantile of the pixels d > 0 at 0.01 (the number 0.0 where no pixel is
 * valid), far = log of torch.quantile of every pixel at 0.99, both exact order statistics with torch's linear interpolation (rank = q (n - 1)
 * as an fp32 product, lerp with the weight < 0.5 switch; the log taken in fp64 and rounded once), then per pixel
 * x = 1 - (log(max(d, 1e-9)) - near) / (far - near + 1e-9) in fp32, clipped to [0, 1], row min(int(256 x), 255) of matplotlib's turbo table
 * (src/utils/color_map.py:11-29), each table byte being uint8 of the fp32 row value times 255.  Degenerate frames follow that arithmetic (all
 * zero: near 0, far -inf, every pixel the last row).  NaN depths are out of contract.  One histogram pass per radix digit covers all frames;
 * the masked subset is selected in place.  Deterministic; no synchronisation.  F <= 65535, H W < 2^31.
 * workspace: the _workspace_bytes value for (F, H, W), read only with depths; 0 for sizes the call refuses.
 * wm_turbo_lut: host only, no device work: the 256 x 3 table bytes, rows r g b. */
size_t wm_video_frames_workspace_bytes(int F, int H, int W);
wm_status wm_video_frames(const float* rgbs, const float* depths, int F, int H, int W, unsigned char* rgb_out, unsigned char* depth_out,
                          float* near_far, void* workspace, size_t workspace_bytes, void* stream);
void wm_turbo_lut(unsigned char out[768]);

/* ---- GLB scene hand-off (csrc/glb.hip): the 3-D view of the demo, convert_predictions_to_glb_scene of src/utils/visual_util.py:208-469 with
 * create_image_mesh (:109-205), in the layout of a glTF 2.0 BIN chunk.  All arrays contiguous on the device unless marked host.
 * image mesh.  mask [S,H,W] bytes (non-zero = in; NULL = every pixel).  A quad at pixel p = y W + x is valid when p, p + W, p + W + 1 and
 *   p + 1 are all in; a pixel is a vertex when it is a corner of a valid quad.  Vertices come in ascending pixel index (np.unique's order),
 *   faces in raster order of the quads, (a, b, c), (a, c, d) for the quad (p, p + W, p + W + 1, p + 1), indices local to the view.
 *   The count entry leaves its scans in the workspace, synchronises the stream ONCE and writes n_vertices[S + 1] and n_quads[S + 1] (host:
 *   per view, the total last).  The pack entry, given the same mask and the untouched workspace, writes the views one after another:
 *   positions [V,3] fp32 (bit copies of points [S,H,W,3]), rgba [V,4] u8 = trunc of the reference's three fp32 roundings
 *   fl(fl(fl(x 255) / 255) 255) of colors [S,H,W,3] with alpha 255, normals_out [V,3] (copies of normals [S,H,W,3]; both NULL for none),
 *   faces [2 Q,3] int32, and bounds [S,6] fp32 = min xyz, max xyz of each view's vertices (+inf, -inf for a view without any).
 *   No atomics and no floating-point accumulation: positions come from prefix sums.  Non-finite positions are out of contract for bounds.
 *   workspace: the _workspace_bytes value for (S, H, W): 4 bytes per pixel + about 32 per 512 pixels; 0 for S, H or W < 1 or S H W >= 2^31.
 * point cloud (visual_util.py:274-298).  The rows i of points / colors [N,3] with mask[i] != 0 (NULL: all), in order: out[0, 12 n) positions,
 *   out[12 n, 16 n) RGBA = trunc(fl(x 255)), alpha 255; out_bytes >= 16 N, 4-byte aligned; bounds [6].  Synchronises once and writes *n_kept
 *   (host) = n.  workspace: the _workspace_bytes value for N; 0 for N < 1 or N >= 2^31.
 * percentile neighbours (np.percentile's selection, visual_util.py:307-308).  For column c of points [N,3] and quantile j (quantiles: host,
 *   1 .. 4 values in [0, 1]) out[(c n_quantiles + j) 2 + u], u = 0, 1: the order statistics of rank floor((n - 1) q_j) + u (clipped to n - 1)
 *   among the n rows with mask[i] != 0, exact, by radix selection (integer histogram adds are its only atomics); *count_out (device) = n;
 *   with n = 0 out is not written.  -0 orders below +0; NaN is out of contract.  No synchronisation.
 *   workspace: the _workspace_bytes value; 0 for N < 0, 3 N >= 2^31 or n_quantiles outside 1 .. 4.
 * WM_ERR_INVALID, before anything is launched: a null pointer where none is allowed, sizes the size calls refuse, a too small workspace or
 *   output buffer, a misaligned output. */
size_t wm_image_mesh_workspace_bytes(int S, int H, int W);
wm_status wm_image_mesh_count(const unsigned char* mask, int S, int H, int W, void* workspace, size_t workspace_bytes, int64_t* n_vertices,
                              int64_t* n_quads, void* stream);
wm_status wm_image_mesh_pack(const float* points, const float* colors, const float* normals, const unsigned char* mask, int S, int H, int W,
                             const void* workspace, size_t workspace_bytes, int64_t total_vertices, int64_t total_quads, float* positions,
                             unsigned char* rgba, float* normals_out, int32_t* faces, float* bounds, void* stream);
size_t wm_glb_pack_points_workspace_bytes(int64_t N);
wm_status wm_glb_pack_points(const float* points, const float* colors, const unsigned char* mask, int64_t N, void* workspace,
                             size_t workspace_bytes, void* out, size_t out_bytes, int64_t* n_kept, float* bounds, void* stream);
size_t wm_masked_percentile_neighbours_workspace_bytes(int64_t N, int n_quantiles);
wm_status wm_masked_percentile_neighbours(const float* points, const unsigned char* mask, int64_t N, const double* quantiles, int n_quantiles,
                                          void* workspace, size_t workspace_bytes, float* out, int64_t* count_out, void* stream);

/* ---- Trainer evaluation (csrc/evalmetrics.hip): Runner.eval of gsplat's simple_trainer_worldmirror.py:1005-1091 and color_correct of
 * examples/lib_bilagrid.py:56-126.  Both entries are asynchronous on stream and never synchronise the host.  Every sum is fp64 in a fixed
 * order (a lane in index order, a block by a fixed tree or one lane per sum, the blocks' partials in block order): no floating-point atomics,
 * results are bitwise reproducible.
 * eval frame (:1040-1054).  colors, pixels: fp32 [B,H,W,3] addressed by ELEMENT strides (sB, sH, sW, sC) (host arrays, read during the call), so
 *   channels 0:3 of an RGB+ED [B,H,W,4] render and the permuted view of a [B,3,H,W] tensor are read in place.  c = clamp(colors, 0, 1) when
 *   clamp_colors (NaN stays NaN), else colors.  clamped_out [B,H,W,3] fp32 contiguous = c.  canvas_out uint8 [B,H,2W,3]: pixels on the left,
 *   c on the right, each byte the fp32 product v * 255.0f truncated toward zero ((canvas * 255).astype(np.uint8); values outside [0, 1] are
 *   out of contract and saturate); it needs clamp_colors.  *psnr_out = 10 log10(data_range^2 / mse) over all B H W 3 values and
 *   psnr_per_image[b] the same over image b, fp32 device values formed in fp64 from differences and squares taken in fp64 of the fp32 inputs;
 *   +inf for mse == 0.  A per-image value does not depend on B.  Any of the four outputs may be NULL.
 *   workspace: the _workspace_bytes value (8 bytes per 1024 pixels of each image), 8-byte aligned; 0 for B, H or W < 1, B > 65535 or
 *   6 H W >= 2^31.
 * colour correction.  img, ref, out: contiguous fp32 [n_systems][n_pixels][3]; each system is fitted on its own (n_systems = 1: the
 *   reference's reshape([-1, 3])).  The reference's algorithm, masks, num_iters and eps; per iteration one pass forms the 10 features of the
 *   current image (rr rg rb gg gb bb r g b 1) and adds, per channel c under mask0_c & unclipped(cur_c) & unclipped(ref_c), the 55 unique
 *   Gram entries and the 10 right-hand sides (products in fp64 of the fp32 values); the blocks' partial sums are added in block order, and one wave per system solves the three 10 x 10
 *   normal equations: cyclic Jacobi eigendecomposition, then the MINIMUM-NORM least-squares solution over the eigenvalues above 1e-10 of
 *   the largest (a channel with an empty mask gets w = 0).  The next pass applies the warp in fp64, clips to [0, 1], rounds the image to
 *   fp32 (once per iteration, as the fp32 reference does) and accumulates again; the last pass only applies.  is_unclipped compares in fp32
 *   against (float)eps and (float)(1 - eps).  num_iters = 0 copies img to out.  out must not overlap img (mask0 is re-read from img).
 *   workspace: the _workspace_bytes value (1560 bytes per 512 pixels of each system + 1800 per system), 8-byte aligned; 0 for
 *   n_systems outside 1 .. 65535 or n_pixels outside 1 .. 2^31 - 1.
 * WM_ERR_INVALID, before anything is launched: a null input or workspace, sizes the size calls refuse, a too small or misaligned workspace,
 *   data_range <= 0, a canvas without clamp_colors, num_iters < 0, eps outside (0, 0.5), out overlapping img. */
size_t wm_eval_frame_workspace_bytes(int B, int H, int W);
wm_status wm_eval_frame(const float* colors, const int64_t* color_strides, const float* pixels, const int64_t* pixel_strides, int B, int H,
                        int W, int clamp_colors, double data_range, float* clamped_out, unsigned char* canvas_out, float* psnr_out,
                        float* psnr_per_image, void* workspace, size_t workspace_bytes, void* stream);
size_t wm_color_correct_workspace_bytes(int n_systems, int64_t n_pixels);
wm_status wm_color_correct(const float* img, const float* ref, int n_systems, int64_t n_pixels, int num_iters, double eps, float* out,
                           void* workspace, size_t workspace_bytes, void* stream);

/* ---- PNG compression of trained splats (csrc/compress.hip): the device side of gsplat.compression.PngCompression
 * (gsplat/compression/png_compression.py) as the trainer's run_compression calls it (simple_trainer_worldmirror.py:1293-1307).  All pointers
 * are device pointers unless said otherwise; no entry synchronises; every entry returns WM_ERR_INVALID before anything is launched for a
 * null pointer (other than the optional ones), a size it refuses or a too small workspace.
 *
 * wm_compress_minmax: mm [2 C] fp32 = the C per-channel minima, then the C maxima, of x [rows, C] (C in 1..16); NaN enters neither.
 *   *nonfinite_flag (one int) is set to 1 when x holds a NaN or an infinity and is otherwise left as it is: the caller zeroes it before the
 *   first call of a batch and reads it once after the last.  Two-level block reduction, no atomics, the same bits on every run.
 * wm_compress_quantise: code = rint(((x - min) / (max - min)) * (2^bits - 1)) in fp32, every operation rounded on its own, the division
 *   IEEE, rint half to even (numpy.round); a channel with max == min encodes as 0 (the reference divides 0 by 0).  bits <= 8: one byte
 *   plane lo [rows, C], hi NULL; bits 9..16: the low bytes in lo and the high bytes in hi.
 * wm_compress_dequantise: out = float(double(code) / (2^bits - 1) * double(float(max - min)) + double(min)), the reference's fp64 decoder,
 *   every operation rounded on its own.  hi NULL exactly when bits <= 8.
 * wm_gather_rows: dst_f[r, :] = src_f[idx[r], :] for r < rows and n_fields <= 16 fields in one launch.  src, dst (arrays of device pointers)
 *   and row_bytes are HOST arrays of n_fields entries; idx [rows] int32 on the device, every value a row of each source (not checked).
 *   A destination must not overlap a source.
 * wm_kmeans_l1: Lloyd's algorithm under Manhattan distance on x [N, D] fp32, D in {9, 24, 45}, 1 <= K <= 65536, K <= N <= 2^30.
 *   The initial centroids are the rows init [K] (int64).  Iteration t: (1) every row goes to the centroid of least L1 distance, the distance an
 *   fp32 sum in the order d = 0 .. D-1, ties to the lowest index; (2) errors[t] = the mean assigned distance (fp64, fixed-order two-level
 *   sum); (3) every centroid with members becomes the mean of its members (summed in row order in fp64, rounded once to fp32), a centroid
 *   without members keeps its value.  The loop ends after max_iter iterations or after the first t > 0 with
 *   |errors[t-1] - errors[t]| <= tol errors[t-1]; the rule is evaluated on the device and the later iterations' kernels return at once.
 *   Then labels [N] int32 = one more assignment against the final centroids [K, D]; labels_last [N] (may be NULL) = the assignment of
 *   the last iteration, whose member means the centroids are.  errors [max_iter] fp64, only the first info[0] written.  info [2] int32:
 *   the iterations run, and 1 when an init row was outside 0 .. N-1 (row 0 was taken; the caller should refuse the result).
 *   No float atomics anywhere: the same input and init give the same bits.  workspace: 20 N + 4 K bytes + the sort's scratch.
 * wm_kmeans_l1_assign: step (1) on its own for x [N, D] (1 <= N <= 2^30) against a given table centroids [K, D]: labels [N] int32 and dist [N]
 *   fp32, the L1 distance to the chosen centroid; the same arithmetic and tie rule, no workspace.
 * wm_grid_order: perm [n_side^2] int32 = the row of means [n_side^2, 3] that goes to every cell (row-major) of the n_side x n_side grid:
 *   the rows in the stable order of their 30-bit Morton codes (per-axis bounding box, 10 bits per axis) are laid along the cells in the
 *   order of the cells' 2-D Morton codes.  Deterministic.  n_side in 1..46340.  nonfinite_flag as above.  workspace: 32 bytes per row + scratch. */
size_t wm_compress_minmax_workspace_bytes(int64_t rows, int C);
wm_status wm_compress_minmax(const float* x, int64_t rows, int C, void* workspace, size_t workspace_bytes, float* mm, int32_t* nonfinite_flag,
                             void* stream);
wm_status wm_compress_quantise(const float* x, int64_t rows, int C, const float* mm, int bits, unsigned char* lo, unsigned char* hi, void* stream);
wm_status wm_compress_dequantise(const unsigned char* lo, const unsigned char* hi, int64_t rows, int C, const float* mm, int bits, float* out,
                                 void* stream);
wm_status wm_gather_rows(const void* const* src, void* const* dst, const int32_t* row_bytes, int n_fields, const int32_t* idx, int64_t rows,
                         void* stream);
size_t wm_kmeans_l1_workspace_bytes(int64_t N, int D, int K);
wm_status wm_kmeans_l1(const float* x, int64_t N, int D, int K, const int64_t* init, int max_iter, double tol, void* workspace,
                       size_t workspace_bytes, int32_t* labels, int32_t* labels_last, float* centroids, double* errors, int32_t* info, void* stream);
wm_status wm_kmeans_l1_assign(const float* x, int64_t N, int D, const float* centroids, int K, int32_t* labels, float* dist, void* stream);
size_t wm_grid_order_workspace_bytes(int n_side);
wm_status wm_grid_order(const float* means, int n_side, void* workspace, size_t workspace_bytes, int32_t* perm, int32_t* nonfinite_flag,
                        void* stream);

/* Process-wide kernel-selection override for tests and A/B tools (no reference counterpart).  The keys are declared once, in
 * WM_TUNE_KEYS (csrc/wm_kernels.h); INTEGRATION.md lists each with its values and its default, in the same order.
 * value -1 restores the default.  Returns 0, or -1 for an unknown key. */
int wm_set_tuning(const char* key, int value);
/* Key "tap_shared" (default 1): the DPT heads' front.  1: the taps are normalised ONCE (LayerNorm without affine) on the caller's stream and one
 * projection GEMM per tap serves every head, each head's LayerNorm affine folded into its projection weights by wm_reserve (W diag(gamma),
 * b + W beta, fp64 on the host, one rounding) — taken when two or more DPT heads are enabled, the call asks for all of them, and every folded
 * weight is finite in the head operand type (|W gamma| <= 65 504 for f16 heads); otherwise, and with 0, every head normalises and projects
 * the taps itself.  The two forms differ by one operand rounding: round(xhat gamma + beta) x round(W) against round(xhat) x round(W gamma). */

/* host helper: fp32 -> 16-bit (round to nearest even), for building test operands */
void wm_host_to_16(const float* in, uint16_t* out, size_t n, int dtype);

#ifdef __cplusplus
}
#endif
#endif
