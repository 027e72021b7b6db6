// The transformer block of the backbone (DINO, frame and global blocks) on the caller's stream, and the GEMM / LayerNorm launch wrappers.
#include "wm_model.h"

namespace wm_host {

wm_status gemm(Ctx& c, int dt, int epi, const void* A, int lda, const void* Wp, int ldw, void* C, int ldc, const float* bias,
               const float* gamma, int M, int N, int K, WmGemmArgs* extra, int prof_kind, bool* ln_fused) {
  WmGemmArgs a;
  if (extra) a = *extra; else memset(&a, 0, sizeof(a));
  a.A = A; a.W = Wp; a.C = C; a.bias = bias; a.gamma = gamma;
  a.M = M; a.N = N; a.K = K; a.lda = lda; a.ldw = ldw; a.ldc = ldc; a.dtype = dt; a.epi = epi;
  // timing kinds by kernel instantiation: the three epilogues that carry the transformer blocks, the rest under PK_GEMM
  ProfScope ps(c.h, prof_kind >= 0 ? prof_kind : epi == WM_EPI_QKV ? PK_GEMM_QKV : epi == WM_EPI_RESID ? PK_GEMM_RESID : epi == WM_EPI_GELU_T16 ? PK_GEMM_GELU : PK_GEMM, c.s);
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

// The overlapped form of a global block's attention in a sharded forward (tuning comm_overlap = 1): fork, attention over the local keys, the
// gather on the communication queue, attention over the remote keys, combine.  a: the site's arguments as attention() below has set them.
// The caller has checked every launch argument set: nothing here may fail between the fork and the collective.
static wm_status attention_overlapped(Ctx& c, WmAttnArgs a, void* K16, void* V16, int M, int heads, size_t hsz, int ntpc, size_t hint_n) {
  wm_handle* h = c.h;
  const Dims& d = c.d;
  const Workspace& ws = h->ws;
  int* const hint0 = a.unit_hint;
  int* const stat0 = a.unit_stat;
  wm_status st;
  // ---- K/V all-gather UNDER the attention over this rank's own keys: the collective runs on the handle's
  // communication queue as soon as the QKV epilogue has written K|V; the compute queue meanwhile attends the local chunk
  // (1 / world of the keys: about the gather's own duration at 8 ranks), then the remote chunks — the gathered buffer's
  // ranges [0, rank) and (rank, world) — and one combine pass over all partial slots.  Softmax partials make the order
  // of the three key ranges irrelevant (attention.hip attn_combine_kernel).
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
    ProfScope ps(h, PK_ATTN_GLOBAL, c.s);
    LCHK(c, wm_launch_attention(a, c.s));
  }
  LCHK(c, hipStreamWaitEvent(h->cstream, h->cfork, 0));
  st = comm_allgather(h, K16, KVG, 2 * hsz, h->cstream);
  if (st) return st;
  LCHK(c, hipEventRecord(h->cjoin, h->cstream));
  LCHK(c, hipStreamWaitEvent(c.s, h->cjoin, 0));
  // (2) remote keys: gathered chunks [0, rank) and (rank, world)
  ProfScope ps(h, PK_ATTN_GLOBAL, c.s);
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
  return WM_OK;
}

// The attention of one block (one call site): the site's fallback policy, then the plain launch, the launch over the gathered K/V of a sharded
// forward, or the overlapped form above
static wm_status attention(Ctx& c, void* Q16, void* K16, void* V16, void* O16, int M, int seq_len, int heads, bool is_global, size_t hsz) {
  wm_handle* h = c.h;
  const Dims& d = c.d;
  const Workspace& ws = h->ws;
  const int dt = c.bdt;
  wm_status st;
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
  if (overlap_ok) return attention_overlapped(c, a, K16, V16, M, heads, hsz, ntpc, hint_n);
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
  ProfScope ps(h, is_global ? PK_ATTN_GLOBAL : PK_ATTN_LOCAL, c.s);
  LCHK(c, wm_launch_attention(a, c.s));
  return WM_OK;
}

// Block.forward (block.py:72-93) on the fp32 residual stream X [M][D]; seq_len = attention span.
// tap_half: when non-null, the block's output (the value its last GEMM stores to X) is also written to tap_half[row * 2D + col]
// by that GEMM's epilogue — the cat([frame_out, global_out], -1) of visual_transformer.py:337-339 without a copy pass.
// next_norm1: norm1 of the block that follows on the same stream X (null = none): it is then computed by this block's fc2
// epilogue when the shape allows (wm_gemm_fuses_ln) and *ln1_ready tells the caller to pass ln1_done to that block.
wm_status backbone_block(Ctx& c, const BlockW& w, float* X, int M, int seq_len, int heads, float eps,
                         bool rope, int tokens_per_view, int patch_start, bool is_global, float* tap_half,
                         bool ln1_done, const Norm* next_norm1, bool* ln1_ready) {
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
  // the residual GEMMs carry the LayerNorm that follows them when the launch allows it (gemm_pp2.hip epilogue_resid_ln)
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
  st = attention(c, Q16, K16, V16, O16, M, seq_len, heads, is_global, hsz);
  if (st) return st;
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

}  // namespace wm_host
