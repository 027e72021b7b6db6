// Splat densification — gsplat's DefaultStrategy (gsplat/strategy/default.py, ops.py), the adaptive density control the reference's
// "Post 3DGS Optimization" trainer runs around every step.  Three calls, no atomics, every sum in a fixed order:
//   accumulate  every step (_update_state, default.py:220-260): one thread per Gaussian walks the cameras in order; where the camera
//               sees it (both radii > 0) it adds the norm of the screen-normalised 2-D mean gradient to grad2d, 1 to count and,
//               on request, raises the running maximum of the normalised screen radius.  index_add_ on the CPU adds in the same
//               (camera-major) order.
//   plan        at a refinement (_grow_gs + _prune_gs, default.py:263-339): classify every Gaussian (duplicate, split), evaluate the
//               prune predicate on every entry duplicate -> split would PRODUCE, on that entry's own values, and lay the survivors
//               out as duplicate -> split -> remove do (ops.py:93-210): un-split originals, duplicates, first split children, second
//               split children, each in index order.  One exclusive scan (rocPRIM through hipCUB) of five flags per Gaussian gives
//               every destination.  Output: per output row the source index, the kind and, for split rows, the parent's rank among
//               the split Gaussians (the row of the noise it uses); the four counts are read back after one stream synchronisation.
//   gather      one [N, R] tensor -> [n_out, R] by the plan: plain copy, Adam moments (new rows zero), means (split children move by
//               R(q) (exp(s) * noise)), scales (split children log(exp(s) / 1.6)), revised opacities (arXiv:2404.06109).
#include "scene_common.h"
#include "wm_kernels.h"

namespace {

struct Flags { unsigned int keep_orig, keep_dup, keep_split, split, dup; };
struct FlagsSum {
  __host__ __device__ Flags operator()(const Flags& a, const Flags& b) const {
    return Flags{a.keep_orig + b.keep_orig, a.keep_dup + b.keep_dup, a.keep_split + b.keep_split, a.split + b.split, a.dup + b.dup};
  }
};

__global__ __launch_bounds__(256) void densify_accumulate_kernel(const float* __restrict__ v_means2d, const int* __restrict__ radii, int N, int C,
                                                                 float sx, float sy, float den, float* __restrict__ grad2d,
                                                                 float* __restrict__ count, float* __restrict__ radii_state) {
  const int g = blockIdx.x * 256 + threadIdx.x;
  if (g >= N) return;
  float acc = grad2d[g], cnt = count[g], rs = radii_state ? radii_state[g] : 0.f;
  for (int c = 0; c < C; ++c) {
    const size_t i = (size_t)c * N + g;
    const int2 r = ((const int2*)radii)[i];
    if (r.x <= 0 || r.y <= 0) continue;
    const float2 v = ((const float2*)v_means2d)[i];
    acc += hypotf(v.x * sx, v.y * sy);
    cnt += 1.0f;
    if (radii_state) rs = fmaxf(rs, (float)max(r.x, r.y) / den);
  }
  grad2d[g] = acc; count[g] = cnt;
  if (radii_state) radii_state[g] = rs;
}

__device__ __forceinline__ float sigmoidf(float x) { return 1.0f / (1.0f + expf(-x)); }

// item N is the all-zero tail, so that the exclusive scan leaves the totals at [N]
__global__ __launch_bounds__(256) void densify_classify_kernel(WmDensifyPlanArgs a, Flags* __restrict__ flags) {
  const int g = blockIdx.x * 256 + threadIdx.x;
  if (g > a.N) return;
  Flags f{0u, 0u, 0u, 0u, 0u};
  if (g < a.N) {
    const float mean_grad = a.grad2d[g] / fmaxf(a.count[g], 1.0f);
    const float smax = fmaxf(fmaxf(expf(a.scales[3 * g]), expf(a.scales[3 * g + 1])), expf(a.scales[3 * g + 2]));
    const float rs = a.use_scale2d ? a.radii_state[g] : 0.f;
    const bool high = mean_grad > a.grow_grad2d, small = smax <= a.grow_scale3d;
    const bool dup = high && small;
    const bool split = (high && !small) || (a.use_scale2d && rs > a.grow_scale2d);
    // an entry's radius state is its parent's (ops.py:118-120, 176-180)
    const bool big2d = a.prune_big && a.use_scale2d && rs > a.prune_scale2d;
    const float op = sigmoidf(a.opacities[g]);
    const bool prune_own = op < a.prune_opa || (a.prune_big && smax > a.prune_scale3d) || big2d;
    const float op_child = a.revised_opacity ? 1.0f - sqrtf(1.0f - op) : op;
    const bool prune_child = op_child < a.prune_opa || (a.prune_big && smax / 1.6f > a.prune_scale3d) || big2d;
    f.split = split; f.dup = dup;
    f.keep_orig = !split && !prune_own;
    f.keep_dup = dup && !prune_own;
    f.keep_split = split && !prune_child;
  }
  flags[g] = f;
}

__global__ __launch_bounds__(256) void densify_scatter_kernel(const Flags* __restrict__ flags, const Flags* __restrict__ excl, int N,
                                                              int* __restrict__ src, int* __restrict__ kind, int* __restrict__ rank,
                                                              int* __restrict__ counts_dev) {
  const int g = blockIdx.x * 256 + threadIdx.x;
  if (g >= N) return;
  const Flags tot = excl[N], f = flags[g], e = excl[g];
  if (g == 0) {
    const unsigned int n_out = tot.keep_orig + tot.keep_dup + 2u * tot.keep_split;
    const unsigned int produced = (unsigned int)N - tot.split + tot.dup + 2u * tot.split;
    counts_dev[0] = (int)tot.dup; counts_dev[1] = (int)tot.split; counts_dev[2] = (int)(produced - n_out); counts_dev[3] = (int)n_out;
  }
  if (f.keep_orig) { const unsigned int d = e.keep_orig; src[d] = g; kind[d] = WM_DENSIFY_KEEP; rank[d] = 0; }
  if (f.keep_dup) { const unsigned int d = tot.keep_orig + e.keep_dup; src[d] = g; kind[d] = WM_DENSIFY_DUP; rank[d] = 0; }
  if (f.keep_split) {
    const unsigned int d0 = tot.keep_orig + tot.keep_dup + e.keep_split, d1 = d0 + tot.keep_split;
    src[d0] = g; kind[d0] = WM_DENSIFY_SPLIT0; rank[d0] = (int)e.split;
    src[d1] = g; kind[d1] = WM_DENSIFY_SPLIT1; rank[d1] = (int)e.split;
  }
}

// one thread per output element.  noise [2, N, 3]: half b, row = the parent's rank among the split Gaussians.
__global__ __launch_bounds__(256) void densify_gather_kernel(const float* __restrict__ in, float* __restrict__ out, int N, int R, int mode,
                                                             const int* __restrict__ src, const int* __restrict__ kind,
                                                             const int* __restrict__ rank, size_t total, const float* __restrict__ quats,
                                                             const float* __restrict__ scales, const float* __restrict__ noise) {
#pragma clang fp contract(off)   // the reference rounds every product before it adds (einsum, then +)
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const size_t row = i / (size_t)R;
  const int col = (int)(i - row * (size_t)R);
  const int g = src[row], k = kind[row];
  float v = in[(size_t)g * R + col];
  const bool child = k == WM_DENSIFY_SPLIT0 || k == WM_DENSIFY_SPLIT1;
  if (mode == WM_GATHER_ZERO_NEW) {
    v = k == WM_DENSIFY_KEEP ? v : 0.f;
  } else if (child && mode == WM_GATHER_MEANS) {
    const float q0 = quats[4 * g], q1 = quats[4 * g + 1], q2 = quats[4 * g + 2], q3 = quats[4 * g + 3];
    const float qn = fmaxf(sqrtf(q0 * q0 + q1 * q1 + q2 * q2 + q3 * q3), 1e-12f);   // F.normalize
    const float w = q0 / qn, x = q1 / qn, y = q2 / qn, z = q3 / qn;
    float r0, r1, r2;                                                               // row `col` of the rotation matrix
    if (col == 0) { r0 = 1.f - 2.f * (y * y + z * z); r1 = 2.f * (x * y - w * z); r2 = 2.f * (x * z + w * y); }
    else if (col == 1) { r0 = 2.f * (x * y + w * z); r1 = 1.f - 2.f * (x * x + z * z); r2 = 2.f * (y * z - w * x); }
    else { r0 = 2.f * (x * z - w * y); r1 = 2.f * (y * z + w * x); r2 = 1.f - 2.f * (x * x + y * y); }
    const float* nz = noise + ((size_t)(k == WM_DENSIFY_SPLIT1 ? N : 0) + (size_t)rank[row]) * 3;
    const float s0 = expf(scales[3 * g]), s1 = expf(scales[3 * g + 1]), s2 = expf(scales[3 * g + 2]);
    v = v + (r0 * s0 * nz[0] + r1 * s1 * nz[1] + r2 * s2 * nz[2]);
  } else if (child && mode == WM_GATHER_SCALES) {
    // the two formulas of a split child in fp64, rounded once: fp32 log (v_log_f32 times ln 2) is an ulp or two off, which on a
    // log scale of magnitude 2-8 is above what torch's fp32 gives; a refinement is cold (every refine_every steps)
    v = (float)log(exp((double)v) / 1.6);
  } else if (child && mode == WM_GATHER_OPACITIES_REVISED) {
    const double sg = 1.0 / (1.0 + exp(-(double)v));
    const double o = 1.0 - sqrt(1.0 - sg);
    v = (float)log(o / (1.0 - o));
  }
  out[i] = v;
}

struct PlanWs { Flags* flags; Flags* excl; int* counts; void* cub; size_t cub_bytes, total; };

PlanWs carve(char* base, size_t N) {
  PlanWs w;
  Carver c(base);
  w.flags = c.take<Flags>(N + 1);
  w.excl = c.take<Flags>(N + 1);
  w.counts = c.take<int>(4);
  w.cub_bytes = exclusive_scan_bytes(FlagsSum(), Flags{0u, 0u, 0u, 0u, 0u}, (int)(N + 1));
  w.cub = c.take<char>(w.cub_bytes);
  w.total = c.total();
  return w;
}

}  // namespace

hipError_t wm_launch_densify_accumulate(const float* v_means2d, const int* radii, int N, int C, int width, int height, float* grad2d,
                                        float* count, float* radii_state, hipStream_t s) {
  if (N <= 0 || C <= 0 || width <= 0 || height <= 0) return hipErrorInvalidValue;
  // default.py:225-226: grads[..., 0] *= width / 2.0 * n_cameras, the factor rounded to fp32 once
  const float sx = (float)((double)width / 2.0 * (double)C), sy = (float)((double)height / 2.0 * (double)C);
  hipLaunchKernelGGL(densify_accumulate_kernel, dim3(blocks_for(N, 256)), dim3(256), 0, s, v_means2d, radii, N, C, sx, sy,
                     (float)(width > height ? width : height), grad2d, count, radii_state);
  return hipGetLastError();
}

size_t wm_densify_plan_ws_bytes(size_t N) { return carve(nullptr, N).total; }

hipError_t wm_launch_densify_plan(const WmDensifyPlanArgs& a, hipStream_t s) {
  if (a.N <= 0 || (size_t)a.N >= (1ull << 29)) return hipErrorInvalidValue;   // 3 N rows are indexed by int
  if (a.use_scale2d && !a.radii_state) return hipErrorInvalidValue;
  PlanWs w = carve((char*)a.workspace, (size_t)a.N);
  if (w.total > a.workspace_bytes) return hipErrorInvalidValue;
  hipLaunchKernelGGL(densify_classify_kernel, dim3(blocks_for(a.N + 1, 256)), dim3(256), 0, s, a, w.flags);
  hipError_t e = exclusive_scan(w.cub, w.cub_bytes, w.flags, w.excl, FlagsSum(), Flags{0u, 0u, 0u, 0u, 0u}, a.N + 1, s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(densify_scatter_kernel, dim3(blocks_for(a.N, 256)), dim3(256), 0, s, w.flags, w.excl, a.N, a.src, a.kind, a.rank, w.counts);
  e = read_back(a.counts, w.counts, 4 * sizeof(int), s);
  if (e != hipSuccess) return e;
  return hipGetLastError();
}

hipError_t wm_launch_densify_gather(const float* in, float* out, int N, int R, int mode, const int* src, const int* kind, const int* rank,
                                    int n_out, const float* quats, const float* scales, const float* noise, hipStream_t s) {
  if (N <= 0 || R <= 0 || n_out < 0 || mode < WM_GATHER_COPY || mode > WM_GATHER_OPACITIES_REVISED) return hipErrorInvalidValue;
  if (mode == WM_GATHER_MEANS && (R != 3 || !quats || !scales || !noise)) return hipErrorInvalidValue;
  if (mode == WM_GATHER_SCALES && R != 3) return hipErrorInvalidValue;
  if (mode == WM_GATHER_OPACITIES_REVISED && R != 1) return hipErrorInvalidValue;
  if (n_out == 0) return hipSuccess;
  const size_t total = (size_t)n_out * (size_t)R;
  if ((total + 255) / 256 >= (1ull << 31)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(densify_gather_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, in, out, N, R, mode, src, kind, rank, total, quats,
                     scales, noise);
  return hipGetLastError();
}
