// Host orchestrator of the MI355X-native WorldMirror forward pass: the forward itself and its C-ABI entries (include/wm_hip.h).
//
// One wm_handle = one process/GPU: owns the repacked weights and a workspace arena, and turns
// WorldMirror.forward (reference src/models/models/worldmirror.py:120-216) into a fixed sequence of
// HIP kernel launches on the caller's stream.  No torch, no hidden per-call allocation once the
// workspace for a shape exists.  The orchestrator's other concerns, each behind wm_model.h: wm_weights.cpp (weight store, lifecycle),
// wm_compose.cpp (composed head weights), wm_plan.cpp (arena, binder, host tables, queues: wm_reserve), wm_comm.cpp (communicator),
// wm_backbone.cpp (transformer block), wm_heads.cpp (camera and DPT heads).  The other entries of the C ABI are in wm_api_ops.cpp (wm_op_*) and
// wm_api_scene.cpp (ingest, masks, rasteriser, densify, MCMC, losses, bilagrid, appearance).
#include "wm_model.h"

using namespace wm_host;

namespace {

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
  // no allocation, no host-side table building, no queue or event creation and no synchronisation in the forward: the workspace must exist
  // (wm_reserve), and with it the heads' queues; the gather's queue comes with the communicator
  if (!(h->plan_n == d.n && h->plan_nt == d.nt && h->plan_H == d.H && h->plan_W == d.W))
    return fail(h, WM_ERR_STATE, "no workspace for this shape: call wm_reserve(h, n_local, n_total, H, W) first (and again after loading weights)");
  wm_status st = WM_OK;
  for (int k = 0; k < wm_handle::NKIND; ++k) h->ev_used[k] = 0;
  ProfScope whole(h, PK_FORWARD, s);
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
  // No kernel outside the GELU instantiations of the gemm_*.hip kernels contains a packed-fp32 instruction any more (-fno-slp-vectorize,
  // WM_NO_PACKED_FP32 in wm_common.h; held by tests/test_kernel_resources_cpu.py, which disassembles every object), and those
  // GELU GEMMs of the backbone have finished before this fork.  tools/stress_concurrent_heads.py: 4 900 concurrent forwards (C2, C3, C5 flag set) bit-identical
  // to the serial one.
  const bool serial = wm_tune(WM_TUNE_HEADS_CONC, 1) == 0 || h->prof;
  if (!serial) LCHK(c, hipEventRecord(h->hfork, s));
  // ---- a11-a12: camera head.  864 MB of fp32 weights streamed 4 times for <= 64 rows: HBM-bound (1.3 ms at 8 views), so it runs
  // on its own queue BESIDE the MFMA-bound DPT heads (which do not depend on it, except the Gaussian head's splat assembly).
  bool cam_async = false;
  if (cf.enable_cam && out->camera_params) {
    Ctx cc = c;
    if (!serial) {
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
      if (!serial) LCHK(c, hipEventRecord(h->hfront, s));
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
