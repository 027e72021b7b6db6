// Point-cloud filter masks of the demo (reference: app.py:172-206 run_model, with depth_edge and
// normals_edge of src/utils/geometry.py:374-416 / 472-531):
//
//   per view i:  conf_mask = conf[i] >= np.quantile(conf[i], p / 100)                       (apply_confidence_mask)
//                edge      = depth_edge(depth[i], rtol, mask) & normals_edge(normals[i], tol, mask)
//                final     = conf_mask & ~edge                                                (apply_edge_mask)
//
// Two parts, both HBM-bound with no matrix work:
//  * the per-view quantile: an exact order-statistic selection (4 x 8-bit radix select as in select.hip, one histogram
//    pair per view: blockIdx.y = view) of the two neighbours numpy's linear method interpolates between, then numpy's
//    own fp32 lerp (numpy 2.2 lib/_function_base_impl.py _quantile / _lerp);
//  * one fused stencil launch over all views x 2-D tiles: normals and mask staged in LDS with a halo of 2r, depth with
//    a halo of r, the stage-1 angle map kept in LDS for the stage-2 pool.
//
// Semantics reproduced from running the reference (none of it is visible from reading it alone):
//  1. normals_edge's mask window is TRANSPOSED: for a 2-D mask, sliding_window_2d(..., axis=(-3, -2)) resolves to the
//     axes (1, 0), so window entry [a][b] reads mask[y-r+b][x-r+a] while the angle term reads normals[y-r+a][x-r+b].
//     A drop-in copies that.  depth_edge's mask has the plain orientation.
//  2. After the fp32 normalisation n / (|n| + 1e-12) the self-dot n.n exceeds 1 for a large share of unit normals, so
//     arccos gives NaN.  Stage 1 (.max(axis=(-2, -1))) propagates NaN; a masked-out window entry contributes 0, not
//     NaN.  Stage 2 (max_pool_2d = NaN padding + np.nanmax) ignores NaN, so an all-NaN window is not an edge.
//  3. Stage 1 pads normals and mask by edge replication; stage 2 and both depth pools pad with NaN and use nanmax
//     (= clipped windows).  Masked depth is where(mask, +-d, -inf): a fully masked window gives diff = -inf.
//  4. NEP 50: atol / rtol are compared in fp32; the angle is promoted to fp64 against np.deg2rad(tol) (an np.float64).
//  5. Exact fp32 arithmetic: |n| = sqrt((x*x + y*y) + z*z), dot = (p0 + p1) + p2, each op correctly rounded, none
//     contracted to an FMA.  HIP's __fmul_rn / __fadd_rn are plain operators that the default -ffp-contract=fast fuses,
//     and its __fsqrt_rn is the native (1 ulp) sqrt, so this file turns contraction off and uses its own f_* helpers.
//
// Stage 1 evaluates one acosf per pixel: acos is non-increasing, so the window maximum of arccos(dot) is
// arccos(min dot) over the unmasked entries; an entry outside [-1, 1] (NaN from arccos) makes the result NaN, and any
// masked entry contributes 0 (<= every arccos value).
#include "scene_common.h"
#include "wm_kernels.h"

#pragma clang fp contract(off)

namespace {

// one correctly rounded IEEE fp32 operation each (contraction is off from here on; fp32 '/' and sqrt are correctly rounded
// under hipcc's default -fhip-fp32-correctly-rounded-divide-sqrt)
__device__ __forceinline__ float f_add(float a, float b) { return a + b; }
__device__ __forceinline__ float f_sub(float a, float b) { return a - b; }
__device__ __forceinline__ float f_mul(float a, float b) { return a * b; }
__device__ __forceinline__ float f_div(float a, float b) { return a / b; }
__device__ __forceinline__ float f_sqrt(float a) { return __builtin_sqrtf(a); }

// ------------------------------------------------------------------ per-view quantile (numpy linear method)
struct QState {
  unsigned int prefix[2];     // bits of the two order statistics fixed so far (high bits)
  unsigned int remaining[2];  // 1-based rank still to find inside the fixed prefix
  unsigned int nan_count;
  unsigned int pad[3];
  unsigned int hist[2][256];
};

// order-preserving uint32 image of an fp32 value; -0 folds onto +0 (numpy orders them as equal), every NaN onto the top
__device__ __forceinline__ unsigned int q_key(float c) {
  if (c != c) return 0xFFFFFFFFu;
  return ordered_key(c == 0.f ? 0.f : c);
}

constexpr int Q_EPT = 16;
constexpr int Q_CHUNK = 256 * Q_EPT;

__global__ __launch_bounds__(256) void q_init_kernel(QState* st, unsigned int lo, unsigned int hi) {
  QState& q = st[blockIdx.x];
  q.hist[0][threadIdx.x] = 0;
  q.hist[1][threadIdx.x] = 0;
  if (threadIdx.x == 0) {
    q.prefix[0] = q.prefix[1] = 0;
    q.remaining[0] = lo + 1;
    q.remaining[1] = hi + 1;
    q.nan_count = 0;
  }
}

// histograms of byte shift/8 of the view's keys whose higher bits equal each target's prefix; grid (blocks, views)
__global__ __launch_bounds__(256) void q_hist_kernel(const float* __restrict__ conf, int n, QState* st, int shift) {
  __shared__ unsigned int lh[2][256];
  __shared__ unsigned int lnan;
  lh[0][threadIdx.x] = 0;
  lh[1][threadIdx.x] = 0;
  if (threadIdx.x == 0) lnan = 0;
  __syncthreads();
  QState& q = st[blockIdx.y];
  const unsigned int p0 = q.prefix[0], p1 = q.prefix[1];
  const unsigned int himask = shift == 24 ? 0u : ~0u << (shift + 8);
  const float* c = conf + (size_t)blockIdx.y * n;
  unsigned int nan = 0;
#pragma unroll
  for (int e = 0; e < Q_EPT; ++e) {
    const int i = blockIdx.x * Q_CHUNK + e * 256 + threadIdx.x;
    if (i < n) {
      const float v = c[i];
      const unsigned int k = q_key(v);
      if ((k & himask) == p0) atomicAdd(&lh[0][(k >> shift) & 255u], 1u);
      if ((k & himask) == p1) atomicAdd(&lh[1][(k >> shift) & 255u], 1u);
      nan += v != v;
    }
  }
  if (shift == 24 && nan) atomicAdd(&lnan, nan);
  __syncthreads();
  if (lh[0][threadIdx.x]) atomicAdd(&q.hist[0][threadIdx.x], lh[0][threadIdx.x]);
  if (lh[1][threadIdx.x]) atomicAdd(&q.hist[1][threadIdx.x], lh[1][threadIdx.x]);
  if (threadIdx.x == 0 && lnan) atomicAdd(&q.nan_count, lnan);
}

// one block per view: walk each target's bins from the bottom; after the last byte, numpy's lerp of the two values
__global__ __launch_bounds__(256) void q_pick_kernel(QState* st, int shift, float gamma, float* __restrict__ thr) {
  __shared__ unsigned int h[2][256];
  QState& q = st[blockIdx.x];
  h[0][threadIdx.x] = q.hist[0][threadIdx.x];
  h[1][threadIdx.x] = q.hist[1][threadIdx.x];
  __syncthreads();
  if (threadIdx.x < 2) {
    const int t = threadIdx.x;
    unsigned int rem = q.remaining[t], bin = 255;
    for (int b = 0; b < 256; ++b) {
      if (h[t][b] >= rem) { bin = (unsigned int)b; break; }
      rem -= h[t][b];
    }
    q.prefix[t] |= bin << shift;
    q.remaining[t] = rem;
  }
  __syncthreads();
  q.hist[0][threadIdx.x] = 0;
  q.hist[1][threadIdx.x] = 0;
  if (shift == 0 && threadIdx.x == 0) {
    // _lerp: diff = b - a; r = a + diff * g, or b - diff * (1 - g) where g >= 0.5, all fp32 (numpy ufuncs: no FMA)
    const float a = ordered_value(q.prefix[0]), b = ordered_value(q.prefix[1]);
    const float d = f_sub(b, a);
    float r = gamma >= 0.5f ? f_sub(b, f_mul(d, f_sub(1.f, gamma))) : f_add(a, f_mul(d, gamma));
    if (q.nan_count) r = __builtin_nanf("");  // NaN sorts last and numpy's result for the slice is NaN
    thr[blockIdx.x] = r;
  }
}

// ------------------------------------------------------------------ fused depth / normal edge stencil
constexpr int PM_TX = 32, PM_TY = 16;  // output tile; 256 threads, 2 pixels per thread

struct PmArgs {
  const float* depth;       // [S][H][W]
  const float* normals;     // [S][H][W][3]
  const unsigned char* mask;  // [S][H][W] or null
  const float* conf;        // [S][H][W] or null: mask = conf >= thr[view]
  const float* thr;         // [S]
  unsigned char* out;       // [S][H][W]
  unsigned char* out_de;    // optional
  unsigned char* out_ne;    // optional
  int S, H, W;
  int do_depth, do_normal, has_atol, has_rtol;
  float atol, rtol;
  double tol_rad;
};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

template <int R>
__global__ __launch_bounds__(256) void point_edge_kernel(const PmArgs a) {
  constexpr int NX = PM_TX + 4 * R, NY = PM_TY + 4 * R;  // normals / mask: halo 2r (edge replicated)
  constexpr int AX = PM_TX + 2 * R, AY = PM_TY + 2 * R;  // stage-1 angle map and depth: halo r (NaN outside the image)
  __shared__ float snx[NY * NX], sny[NY * NX], snz[NY * NX];
  __shared__ unsigned char smk[NY * NX];
  __shared__ float sang[AY * AX], sdp[AY * AX], sdn[AY * AX];

  const int H = a.H, W = a.W, v = blockIdx.z;
  const int tx0 = blockIdx.x * PM_TX, ty0 = blockIdx.y * PM_TY;
  const size_t vbase = (size_t)v * H * W;
  const bool has_mask = a.mask || a.conf;
  const float thr = a.conf ? a.thr[v] : 0.f;

  // stage normals (normalised) and mask, origin (ty0 - 2r, tx0 - 2r), coordinates clamped = np.pad(mode="edge")
  for (int i = threadIdx.x; i < NY * NX; i += 256) {
    const int ly = i / NX, lx = i - ly * NX;
    const int gy = clampi(ty0 - 2 * R + ly, 0, H - 1), gx = clampi(tx0 - 2 * R + lx, 0, W - 1);
    const size_t p = vbase + (size_t)gy * W + gx;
    if (has_mask) smk[i] = a.conf ? (a.conf[p] >= thr ? 1 : 0) : (a.mask[p] ? 1 : 0);
    if (a.do_normal) {
      const float x = a.normals[3 * p], y = a.normals[3 * p + 1], z = a.normals[3 * p + 2];
      const float nrm = f_add(f_sqrt(f_add(f_add(f_mul(x, x), f_mul(y, y)), f_mul(z, z))), 1e-12f);
      snx[i] = f_div(x, nrm);
      sny[i] = f_div(y, nrm);
      snz[i] = f_div(z, nrm);
    }
  }
  __syncthreads();

  if (a.do_normal) {  // stage 1 on (ty0 - r .. ty0 + TY + r) x (tx0 - r ..): max over the window of where(mask_T, arccos(dot), 0)
    for (int i = threadIdx.x; i < AY * AX; i += 256) {
      const int ly = i / AX, lx = i - ly * AX;
      const int gy = ty0 - R + ly, gx = tx0 - R + lx;
      float ang = __builtin_nanf("");  // outside the image: NaN padding of the stage-2 pool
      if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
        const int c = (ly + R) * NX + lx + R;
        const float cx = snx[c], cy = sny[c], cz = snz[c];
        float dmin = INFINITY;
        bool bad = false, any_on = false;
#pragma unroll
        for (int p = 0; p < 2 * R + 1; ++p) {
#pragma unroll
          for (int q = 0; q < 2 * R + 1; ++q) {
            // angle term at normals[y-r+p][x-r+q]; mask term transposed: mask[y-r+q][x-r+p] (see header, item 1)
            if (has_mask && !smk[(ly + q) * NX + lx + p]) continue;  // where(mask, ., 0): 0 <= every arccos
            const int w = (ly + p) * NX + lx + q;
            const float d = f_add(f_add(f_mul(cx, snx[w]), f_mul(cy, sny[w])), f_mul(cz, snz[w]));
            bad |= !(d >= -1.f && d <= 1.f);
            dmin = d < dmin ? d : dmin;
            any_on = true;
          }
        }
        ang = bad ? __builtin_nanf("") : (any_on ? acosf(dmin) : 0.f);
      }
      sang[i] = ang;
    }
  }
  if (a.do_depth) {  // depth with halo r, origin (ty0 - r, tx0 - r): where(mask, +-d, -inf), NaN outside the image
    for (int i = threadIdx.x; i < AY * AX; i += 256) {
      const int ly = i / AX, lx = i - ly * AX;
      const int gy = ty0 - R + ly, gx = tx0 - R + lx;
      float dp = __builtin_nanf(""), dn = __builtin_nanf("");
      if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
        const float d = a.depth[vbase + (size_t)gy * W + gx];
        const bool on = !has_mask || smk[(ly + R) * NX + lx + R];
        dp = on ? d : -INFINITY;
        dn = on ? -d : -INFINITY;
      }
      sdp[i] = dp;
      sdn[i] = dn;
    }
  }
  __syncthreads();

  for (int i = threadIdx.x; i < PM_TY * PM_TX; i += 256) {
    const int ly = i / PM_TX, lx = i - ly * PM_TX;
    const int gy = ty0 + ly, gx = tx0 + lx;
    if (gy >= H || gx >= W) continue;
    const size_t p = vbase + (size_t)gy * W + gx;
    bool de = false, ne = false;
    if (a.do_normal) {  // stage 2: nanmax over the clipped window (fmaxf drops NaN; all-NaN stays NaN)
      float m = __builtin_nanf("");
#pragma unroll
      for (int p2 = 0; p2 < 2 * R + 1; ++p2)
#pragma unroll
        for (int q2 = 0; q2 < 2 * R + 1; ++q2) m = fmaxf(m, sang[(ly + p2) * AX + lx + q2]);
      ne = (double)m > a.tol_rad;
    }
    if (a.do_depth) {
      float mp = __builtin_nanf(""), mn = __builtin_nanf("");
#pragma unroll
      for (int p2 = 0; p2 < 2 * R + 1; ++p2)
#pragma unroll
        for (int q2 = 0; q2 < 2 * R + 1; ++q2) {
          mp = fmaxf(mp, sdp[(ly + p2) * AX + lx + q2]);
          mn = fmaxf(mn, sdn[(ly + p2) * AX + lx + q2]);
        }
      const float diff = f_add(mp, mn);
      if (a.has_atol) de |= diff > a.atol;
      if (a.has_rtol) de |= f_div(diff, a.depth[p]) > a.rtol;
    }
    unsigned char o;
    if (a.do_depth && a.do_normal) o = (has_mask ? smk[(ly + 2 * R) * NX + lx + 2 * R] : 1) & !(de && ne);
    else if (a.do_depth) o = de;
    else if (a.do_normal) o = ne;
    else o = has_mask ? smk[(ly + 2 * R) * NX + lx + 2 * R] : 1;
    a.out[p] = o;
    if (a.out_de) a.out_de[p] = de;
    if (a.out_ne) a.out_ne[p] = ne;
  }
}

hipError_t launch_point_edge(const PmArgs& a, int k, hipStream_t s) {
  if (a.S == 0 || a.H == 0 || a.W == 0) return hipSuccess;
  const dim3 grid((unsigned)((a.W + PM_TX - 1) / PM_TX), (unsigned)((a.H + PM_TY - 1) / PM_TY), (unsigned)a.S);
  switch (k) {
    case 3: hipLaunchKernelGGL(point_edge_kernel<1>, grid, dim3(256), 0, s, a); break;
    case 5: hipLaunchKernelGGL(point_edge_kernel<2>, grid, dim3(256), 0, s, a); break;
    case 7: hipLaunchKernelGGL(point_edge_kernel<3>, grid, dim3(256), 0, s, a); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

bool pm_shape_ok(int S, int H, int W, int k) {
  if (S < 0 || H < 0 || W < 0 || S > 65535) return false;
  if (k != 3 && k != 5 && k != 7) return false;
  return (long long)S * H * W < (1LL << 31);
}

}  // namespace

hipError_t wm_launch_depth_edge(const float* depth, const unsigned char* mask, int S, int H, int W, int k, int has_atol, float atol,
                                int has_rtol, float rtol, unsigned char* out, hipStream_t s) {
  if (!pm_shape_ok(S, H, W, k)) return hipErrorInvalidValue;
  PmArgs a{};
  a.depth = depth; a.mask = mask; a.out = out;
  a.S = S; a.H = H; a.W = W;
  a.do_depth = 1; a.has_atol = has_atol; a.has_rtol = has_rtol; a.atol = atol; a.rtol = rtol;
  return launch_point_edge(a, k, s);
}

hipError_t wm_launch_normals_edge(const float* normals, const unsigned char* mask, int S, int H, int W, int k, double tol_deg,
                                  unsigned char* out, hipStream_t s) {
  if (!pm_shape_ok(S, H, W, k)) return hipErrorInvalidValue;
  PmArgs a{};
  a.normals = normals; a.mask = mask; a.out = out;
  a.S = S; a.H = H; a.W = W;
  a.do_normal = 1;
  a.tol_rad = tol_deg * (3.14159265358979323846 / 180.0);  // np.deg2rad: x * (NPY_PI / 180.0), fp64
  return launch_point_edge(a, k, s);
}

size_t wm_point_filter_mask_workspace(int S, int H, int W) {
  (void)H; (void)W;
  return (size_t)(S > 0 ? S : 0) * (sizeof(QState) + sizeof(float)) + 256;
}

hipError_t wm_launch_point_filter_mask(const float* conf, const float* depth, const float* normals, int S, int H, int W, int apply_conf,
                                       double percentile, int apply_edge, double normal_tol_deg, float depth_rtol,
                                       float* thresholds_out, unsigned char* mask_out, unsigned char* out_de, unsigned char* out_ne,
                                       void* ws, hipStream_t s) {
  if (!pm_shape_ok(S, H, W, 3)) return hipErrorInvalidValue;
  if (S == 0 || H == 0 || W == 0) return hipSuccess;
  const int n = H * W;
  float* thr = nullptr;
  if (apply_conf) {
    if (!(percentile >= 0.0 && percentile <= 100.0)) return hipErrorInvalidValue;  // np.quantile: q in [0, 1]
    // np.quantile(a, p / 100.0) with a float32: q is cast to float32 and the linear method's virtual index (n - 1) * q is a
    // float32 product (NEP 50: the Python int n - 1 is weak); floor / +1 give the two neighbours, gamma = index - floor
    // (computed in fp64 against the intp index, stored as fp32).  At or beyond the last index both neighbours are the last.
    const float q = (float)(percentile / 100.0);
    const float vi = (float)(n - 1) * q;
    unsigned int lo, hi;
    double prev;
    if ((double)vi >= (double)(n - 1)) { lo = hi = (unsigned int)(n - 1); prev = -1.0; }
    else { prev = std::floor((double)vi); lo = (unsigned int)prev; hi = lo + 1; }
    const float gamma = (float)((double)vi - prev);
    QState* st = (QState*)ws;
    thr = thresholds_out ? thresholds_out : (float*)((char*)ws + (size_t)S * sizeof(QState));
    const unsigned int nblk = (unsigned int)((n + Q_CHUNK - 1) / Q_CHUNK);
    hipLaunchKernelGGL(q_init_kernel, dim3(S), dim3(256), 0, s, st, lo, hi);
    for (int shift = 24; shift >= 0; shift -= 8) {
      hipLaunchKernelGGL(q_hist_kernel, dim3(nblk, S), dim3(256), 0, s, conf, n, st, shift);
      hipLaunchKernelGGL(q_pick_kernel, dim3(S), dim3(256), 0, s, st, shift, gamma, thr);
    }
  }
  // app.py: without the confidence mask the edge masks run with mask=None
  PmArgs a{};
  a.depth = depth; a.normals = normals; a.conf = apply_conf ? conf : nullptr; a.thr = thr;
  a.out = mask_out; a.out_de = out_de; a.out_ne = out_ne;
  a.S = S; a.H = H; a.W = W;
  a.do_depth = a.do_normal = apply_edge ? 1 : 0;
  a.has_rtol = 1; a.rtol = depth_rtol;
  a.tol_rad = normal_tol_deg * (3.14159265358979323846 / 180.0);
  return launch_point_edge(a, 3, s);
}
