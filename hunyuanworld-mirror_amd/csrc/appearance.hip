// Appearance optimisation of the post-3DGS trainer: gsplat's AppearanceOptModule (examples/utils.py:51-114), a per-image embedding and a
// small MLP evaluated for every (camera, Gaussian) pair, which simple_trainer_worldmirror.py runs under --app_opt (:532-552 builds it,
// :603-611 calls it).  Built for the trainer's configuration: 32 Gaussian features, 16 embedding values, (Lm + 1)^2 <= 16 SH basis values
// of the viewing direction, Linear 64 / ReLU / Linear 64 / ReLU / Linear 3.  Everything is fp32; the matrix products run on the exact
// fp32-input MFMA (v_mfma_f32_32x32x2_f32: bit for bit a k-ordered fmaf chain).
//
// Orientation.  A wave owns 32 Gaussians; every product is written transposed, OUT^T [64 x 32 pairs] = W [64 x k] . IN^T [k x 32 pairs]:
// the weights are the A operand (read from LDS), the activations the B operand.  A 32 x 32 result has its pair on the lane and its 16
// rows in registers (row = 8 (r / 4) + 4 (lane / 32) + r % 4), which is what the B operand of the next product wants once the k order
// is permuted to match: step (tile, r) takes register r of each lane as B and the weight column of THAT lane half's row as A.  So
// activations never leave registers between the layers.  Only the weight gradients, which sum over the pairs (the lane index), go
// through a transpose in LDS, [row][pair] with stride 33.
//   forward   a block = 4 waves = 128 Gaussians, cameras in an inner loop.  Per tile the feature share of layer 1, W1[:, 16:48] . f, is
//             computed once (32 steps) and kept; per camera the embedding share W1[:, :16] . embed[c] + b1 is 64 numbers computed once
//             by the block, the basis share is 8 steps, layer 2 is 64 MFMAs, layer 3 (3 rows) is 96 FMAs per lane and one exchange
//             between the lane halves.  Nothing of size [C,N,64] is written.
//   backward  recomputes the activations per pair (the feature share too, from the tile's LDS copy: its 32 registers are needed).
//             v_features: the wave that owns the Gaussian sums over the cameras in order, one writer.  v_dirs: W1's basis columns^T .
//             dz1 through sh_basis_vjp and the normalisation.  Weight gradients: a persistent grid whose size depends on N only; a
//             block walks a contiguous run of 128-Gaussian tiles, its waves keep dW2 (64 x 64) and dW1's feature and basis columns
//             (64 x 48) in 128 accumulator registers over the whole run (dW3, three rows, and the bias sums as plain sums), then add
//             them in wave order in LDS and write ONE partial set (7428 floats) to the workspace; per camera the sum of dz1 over the
//             wave's pairs goes to a slot of its own.
//   reduce    adds the blocks' partials in block order, in fp64, rounded once; finalize: b1.grad, the embedding columns of W1.grad and
//             embeds.grad out of the per-camera sums, in camera order (a repeated id is summed deterministically).
// No atomics; every sum runs in a fixed order: identical bits run to run.
#include "wm_common.h"
#include "wm_kernels.h"
#include "sh_basis.h"

using namespace wm_sh;

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int HID = 64, FEAT = 32, EMB = 16, NSH = 16;
constexpr int WS = 65;                 // LDS row stride of W1 / W2: rows and columns are both read conflict-free
constexpr int TS = 33;                 // stride of a transposed [row][pair] tile
constexpr int WAVE_G = 32, BLOCK_G = WM_APPEARANCE_TILE, MAX_BLOCKS = WM_APPEARANCE_MAX_BLOCKS;
// one block's partial set: dW2 [64][64] | dW1 feature + basis columns [64][48] | dW3 [3][64] | db2 [64] | db3 [3] + pad
constexpr int P_W2 = 0, P_W1 = 4096, P_W3 = 4096 + 3072, P_B2 = P_W3 + 192, P_B3 = P_B2 + 64, P_SIZE = P_B3 + 4;
constexpr int T_WAVE = (HID + HID + FEAT + NSH) * TS + 128;   // floats of LDS per wave in the backward: TA | TB | TI | TD
constexpr int W_FLOATS = 2 * HID * WS + 3 * HID + HID + 4 + HID;   // W1s | W2s | W3s | b2s | b3s | e1s

__device__ __forceinline__ f32x16 mfma(float a, float b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0); }
__device__ __forceinline__ constexpr int drow(int r, int half) { return 8 * (r >> 2) + 4 * half + (r & 3); }
// LDS traffic between the lanes of ONE wave: orders this wave's earlier LDS accesses before its later ones
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// half ? hi : lo on the VALUES (a select between two elements of a register array may otherwise be turned into an indexed load, which
// sends the array to scratch)
__device__ __forceinline__ float half_select(int half, float lo, float hi) {
  const unsigned int m = 0u - (unsigned int)half;
  return __uint_as_float((__float_as_uint(hi) & m) | (__float_as_uint(lo) & ~m));
}

struct Lds {
  float* W1s; float* W2s; float* W3s; float* b2s; float* b3s; float* e1s;
};
__device__ __forceinline__ Lds carve_lds(float* base) {
  Lds l;
  l.W1s = base; l.W2s = l.W1s + HID * WS; l.W3s = l.W2s + HID * WS; l.b2s = l.W3s + 3 * HID; l.b3s = l.b2s + HID; l.e1s = l.b3s + 4;
  return l;
}

// weights into LDS.  W1's columns are permuted: [0,32) features (module columns 16..47), [32,48) basis (48..), [48,64) embedding (0..15);
// basis columns the module does not have (its degree below 3) are zeros.
__device__ __forceinline__ void stage_weights(const WmAppearanceArgs& a, const Lds& l) {
  const int in_dim = EMB + FEAT + a.n_bases;
  for (int idx = threadIdx.x; idx < HID * HID; idx += 256) {
    const int i = idx >> 6, k = idx & 63, orig = k < 48 ? k + 16 : k - 48;
    l.W1s[i * WS + k] = orig < in_dim ? a.W1[i * in_dim + orig] : 0.f;
    l.W2s[i * WS + k] = a.W2[idx];
  }
  if (threadIdx.x < 3 * HID) l.W3s[threadIdx.x] = a.W3[threadIdx.x];
  if (threadIdx.x < HID) l.b2s[threadIdx.x] = a.b2[threadIdx.x];
  if (threadIdx.x < 3) l.b3s[threadIdx.x] = a.b3[threadIdx.x];
}

// the embedding row of camera c, or null (embed_ids null, or an id outside [0, n_embeds): a zero embedding)
__device__ __forceinline__ const float* embed_row(const WmAppearanceArgs& a, int c) {
  if (!a.embed_ids) return nullptr;
  const int id = a.embed_ids[c];
  return id >= 0 && id < a.n_embeds ? a.embeds + (size_t)id * EMB : nullptr;
}

// e1s[i] = b1[i] + W1[i, :16] . embed[c]: layer 1's per-camera constant, by threads 0..63 between two block barriers
__device__ __forceinline__ void camera_constant(const WmAppearanceArgs& a, const Lds& l, int c) {
  __syncthreads();
  if (threadIdx.x < HID) {
    const float* e = embed_row(a, c);
    float v = a.b1[threadIdx.x];
    if (e) {
#pragma unroll
      for (int k = 0; k < EMB; ++k) v = fmaf(l.W1s[threadIdx.x * WS + 48 + k], e[k], v);
    }
    l.e1s[threadIdx.x] = v;
  }
  __syncthreads();
}

// F = W1[:, features] . f for the wave's 32 Gaussians; fv: the lane's 16 features [half * 16, half * 16 + 16)
__device__ __forceinline__ void feature_share(const Lds& l, const float* fv, int j, int half, f32x16* F) {
#pragma unroll
  for (int mt = 0; mt < 2; ++mt)
#pragma unroll
    for (int r = 0; r < 16; ++r) F[mt][r] = 0.f;
#pragma unroll
  for (int s = 0; s < 16; ++s)
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) F[mt] = mfma(l.W1s[(mt * 32 + j) * WS + half * 16 + s], fv[s], F[mt]);
}

// layers 1 and 2 of one camera: Z <- h1 = relu(F + W1[:, basis] . B + e1), Y <- h2 = relu(W2 . h1 + b2)
template <int L>
__device__ __forceinline__ void hidden_layers(const Lds& l, const f32x16* F, const float* B, int j, int half, f32x16* Z, f32x16* Y) {
  constexpr int STEPS = L == 0 ? 1 : L == 1 ? 4 : 8;   // basis values (L + 1)^2 and up are zero: their steps add nothing
  Z[0] = F[0]; Z[1] = F[1];
#pragma unroll
  for (int s = 0; s < STEPS; ++s) {
    const float b = half_select(half, B[s], B[8 + s]);
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) Z[mt] = mfma(l.W1s[(mt * 32 + j) * WS + 32 + half * 8 + s], b, Z[mt]);
  }
#pragma unroll
  for (int mt = 0; mt < 2; ++mt)
#pragma unroll
    for (int r = 0; r < 16; ++r) { Z[mt][r] = fmaxf(Z[mt][r] + l.e1s[mt * 32 + drow(r, half)], 0.f); Y[mt][r] = 0.f; }
#pragma unroll
  for (int kt = 0; kt < 2; ++kt)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int k = kt * 32 + drow(r, half);
#pragma unroll
      for (int mt = 0; mt < 2; ++mt) Y[mt] = mfma(l.W2s[(mt * 32 + j) * WS + k], Z[kt][r], Y[mt]);
    }
#pragma unroll
  for (int mt = 0; mt < 2; ++mt)
#pragma unroll
    for (int r = 0; r < 16; ++r) Y[mt][r] = fmaxf(Y[mt][r] + l.b2s[mt * 32 + drow(r, half)], 0.f);
}

// the lane's direction: unit vector d / max(|d|, 1e-12) (F.normalize), its denominator, the basis values (zeros from (L + 1)^2 on)
template <int L>
__device__ __forceinline__ void direction_basis(const float* __restrict__ d, float& x, float& y, float& z, float& den, float* B) {
  const float dx = d[0], dy = d[1], dz = d[2];
  den = fmaxf(sqrtf(dx * dx + dy * dy + dz * dz), 1e-12f);
  x = dx / den; y = dy / den; z = dz / den;
#pragma unroll
  for (int k = 0; k < NSH; ++k) B[k] = 0.f;
  sh_basis<L>(x, y, z, B);
}

__device__ __forceinline__ void load_features(const float* __restrict__ features, int g, bool valid, int half, float* fv) {
  const float4* src = (const float4*)(features + (size_t)g * FEAT + half * 16);
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const float4 v = valid ? src[q] : make_float4(0.f, 0.f, 0.f, 0.f);
    fv[4 * q] = v.x; fv[4 * q + 1] = v.y; fv[4 * q + 2] = v.z; fv[4 * q + 3] = v.w;
  }
}

template <int L>
__global__ __launch_bounds__(256) void appearance_fwd_kernel(WmAppearanceArgs a, float* __restrict__ out) {
  __shared__ float smem[W_FLOATS];
  const Lds l = carve_lds(smem);
  stage_weights(a, l);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, j = lane & 31, half = lane >> 5;
  const int g0 = blockIdx.x * BLOCK_G + wave * WAVE_G + j;
  const bool valid = g0 < a.N;
  const int g = valid ? g0 : a.N - 1;
  float fv[16];
  load_features(a.features, g, valid, half, fv);
  __syncthreads();
  f32x16 F[2], Z[2], Y[2];
  feature_share(l, fv, j, half, F);
  for (int c = 0; c < a.C; ++c) {
    camera_constant(a, l, c);
    const size_t pair = (size_t)c * a.N + g;
    float x, y, z, den, B[NSH];
    direction_basis<L>(a.dirs + 3 * pair, x, y, z, den, B);
    hidden_layers<L>(l, F, B, j, half, Z, Y);
    float o[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int kt = 0; kt < 2; ++kt)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int k = kt * 32 + drow(r, half);
#pragma unroll
        for (int t = 0; t < 3; ++t) o[t] = fmaf(l.W3s[t * HID + k], Y[kt][r], o[t]);
      }
#pragma unroll
    for (int t = 0; t < 3; ++t) o[t] = o[t] + __shfl_xor(o[t], 32) + l.b3s[t];
    if (valid && half == 0) { out[3 * pair] = o[0]; out[3 * pair + 1] = o[1]; out[3 * pair + 2] = o[2]; }
  }
}

template <int L>
__global__ __launch_bounds__(256) void appearance_bwd_kernel(WmAppearanceArgs a, const float* __restrict__ v_out, float* __restrict__ v_features,
                                                             float* __restrict__ v_dirs, float* __restrict__ part, float* __restrict__ part_s1,
                                                             int tiles_per_block) {
  extern __shared__ __attribute__((aligned(16))) float dsm[];
  const Lds l = carve_lds(dsm);
  stage_weights(a, l);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, j = lane & 31, half = lane >> 5;
  float* const tbase = dsm + W_FLOATS;
  float* const TA = tbase + wave * T_WAVE;      // [64][33]: h2, then dz2, then dz1, transposed for the products that sum over pairs
  float* const TB = TA + HID * TS;              // [64][33]: h1
  float* const TI = TB + HID * TS;              // [48][33]: layer 1's inputs: features (per tile), basis (per camera)
  float* const TD = TI + (FEAT + NSH) * TS;     // [32][4]: v_out of the wave's pairs
  f32x16 DW2[4], DW1[4];
#pragma unroll
  for (int q = 0; q < 4; ++q)
#pragma unroll
    for (int r = 0; r < 16; ++r) { DW2[q][r] = 0.f; DW1[q][r] = 0.f; }
  float db2 = 0.f, db3[3] = {0.f, 0.f, 0.f}, dw3[3] = {0.f, 0.f, 0.f};   // db2, dw3: lane = hidden unit; db3: the lane's own pairs
  __syncthreads();
  for (int t = 0; t < tiles_per_block; ++t) {
    const long long g0 = ((long long)blockIdx.x * tiles_per_block + t) * BLOCK_G + wave * WAVE_G + j;
    const bool valid = g0 < a.N;
    const int g = valid ? (int)g0 : a.N - 1;
    float fv[16];
    load_features(a.features, g, valid, half, fv);
    wave_lds_sync();
#pragma unroll
    for (int s = 0; s < 16; ++s) TI[(half * 16 + s) * TS + j] = fv[s];
    float vf[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) vf[r] = 0.f;
    for (int c = 0; c < a.C; ++c) {
      camera_constant(a, l, c);
      const size_t pair = (size_t)c * a.N + g;
      float x, y, z, den, B[NSH];
      direction_basis<L>(a.dirs + 3 * pair, x, y, z, den, B);
      // the feature share is recomputed per camera from the tile's LDS copy: keeping it would cost 32 registers beside the 128 accumulators
      f32x16 F[2], Z[2], Y[2];
      {
        float fc[16];
#pragma unroll
        for (int s = 0; s < 16; ++s) fc[s] = TI[(half * 16 + s) * TS + j];
        feature_share(l, fc, j, half, F);
      }
      hidden_layers<L>(l, F, B, j, half, Z, Y);
      float dout[3];
#pragma unroll
      for (int q = 0; q < 3; ++q) dout[q] = valid ? v_out[3 * pair + q] : 0.f;
      // transposes: TB <- h1, TA <- h2, TI's basis rows, TD <- v_out
      wave_lds_sync();
#pragma unroll
      for (int s = 0; s < 8; ++s) TI[(FEAT + half * 8 + s) * TS + j] = half_select(half, B[s], B[8 + s]);
#pragma unroll
      for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          TB[(mt * 32 + drow(r, half)) * TS + j] = Z[mt][r];
          TA[(mt * 32 + drow(r, half)) * TS + j] = Y[mt][r];
        }
      if (half == 0) { TD[4 * j] = dout[0]; TD[4 * j + 1] = dout[1]; TD[4 * j + 2] = dout[2]; TD[4 * j + 3] = 0.f; }
      wave_lds_sync();
      // dW3 [o][i] += sum_p v_out[p][o] h2[i][p], lane = i: three rows only, so plain FMAs over the transposed tile
      {
        float t3[3] = {0.f, 0.f, 0.f};
#pragma unroll
        for (int p = 0; p < 32; ++p) {
          const float h = TA[lane * TS + p];
          const float4 d = *(const float4*)(TD + 4 * p);
          t3[0] = fmaf(h, d.x, t3[0]); t3[1] = fmaf(h, d.y, t3[1]); t3[2] = fmaf(h, d.z, t3[2]);
        }
        dw3[0] += t3[0]; dw3[1] += t3[1]; dw3[2] += t3[2];
      }
      if (half == 0) { db3[0] += dout[0]; db3[1] += dout[1]; db3[2] += dout[2]; }
      unsigned int relu1 = 0u;   // bit 16 mt + r: h1 > 0
#pragma unroll
      for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int r = 0; r < 16; ++r) relu1 |= Z[mt][r] > 0.f ? 1u << (16 * mt + r) : 0u;
      // dz2 = (h2 > 0) W3^T v_out
#pragma unroll
      for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int k = mt * 32 + drow(r, half);
          const float v = fmaf(l.W3s[2 * HID + k], dout[2], fmaf(l.W3s[HID + k], dout[1], l.W3s[k] * dout[0]));
          Y[mt][r] = Y[mt][r] > 0.f ? v : 0.f;
        }
      wave_lds_sync();
#pragma unroll
      for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int r = 0; r < 16; ++r) TA[(mt * 32 + drow(r, half)) * TS + j] = Y[mt][r];
      wave_lds_sync();
      // dW2 [i][k] += sum_p dz2[i][p] h1[k][p];  db2[i] += sum_p dz2[i][p] (lane = i)
#pragma unroll 2
      for (int s = 0; s < 16; ++s) {
        const int p = 2 * s + half;
        const float a0 = TA[j * TS + p], a1 = TA[(32 + j) * TS + p], b0 = TB[j * TS + p], b1 = TB[(32 + j) * TS + p];
        DW2[0] = mfma(a0, b0, DW2[0]); DW2[1] = mfma(a0, b1, DW2[1]); DW2[2] = mfma(a1, b0, DW2[2]); DW2[3] = mfma(a1, b1, DW2[3]);
      }
      {
        float sum = 0.f;
#pragma unroll
        for (int p = 0; p < 32; ++p) sum += TA[lane * TS + p];
        db2 += sum;
      }
      // dz1 = (h1 > 0) W2^T dz2
      f32x16 D1[2];
#pragma unroll
      for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int r = 0; r < 16; ++r) D1[mt][r] = 0.f;
#pragma unroll
      for (int kt = 0; kt < 2; ++kt)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int k = kt * 32 + drow(r, half);
#pragma unroll
          for (int mt = 0; mt < 2; ++mt) D1[mt] = mfma(l.W2s[k * WS + mt * 32 + j], Y[kt][r], D1[mt]);
        }
#pragma unroll
      for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int r = 0; r < 16; ++r) D1[mt][r] = (relu1 >> (16 * mt + r)) & 1u ? D1[mt][r] : 0.f;
      // gradient of layer 1's inputs, W1^T dz1: tile 0 the 32 features, tile 1 rows 0..15 the basis values (rows 16..31: the embedding, unused)
      f32x16 DI;   // one tile at a time
#pragma unroll
      for (int mt = 0; mt < 2; ++mt) {
#pragma unroll
        for (int r = 0; r < 16; ++r) DI[r] = 0.f;
#pragma unroll
        for (int kt = 0; kt < 2; ++kt)
#pragma unroll
          for (int r = 0; r < 16; ++r) DI = mfma(l.W1s[(kt * 32 + drow(r, half)) * WS + mt * 32 + j], D1[kt][r], DI);
        if (mt == 0) {
#pragma unroll
          for (int r = 0; r < 16; ++r) vf[r] += DI[r];
        }
      }
      if constexpr (L >= 1) {
        // the 16 basis cotangents of the pair: registers 0..7 of this lane hold rows {0-3, 8-11} + 4 half, the other half's lane the rest
        float w[NSH], vd[3];
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          const float mine = DI[q], other = __shfl_xor(mine, 32);
          const int lo = 8 * (q >> 2) + (q & 3);
          w[lo] = half ? other : mine; w[lo + 4] = half ? mine : other;
        }
        sh_basis_vjp<L>(x, y, z, w, vd);
        const float dot = x * vd[0] + y * vd[1] + z * vd[2];   // through d / max(|d|, 1e-12)
        if (valid && half == 0) {
          v_dirs[3 * pair] = (vd[0] - x * dot) / den; v_dirs[3 * pair + 1] = (vd[1] - y * dot) / den; v_dirs[3 * pair + 2] = (vd[2] - z * dot) / den;
        }
      } else {
        if (valid && half == 0) { v_dirs[3 * pair] = 0.f; v_dirs[3 * pair + 1] = 0.f; v_dirs[3 * pair + 2] = 0.f; }
      }
      // dW1 [i][m] += sum_p dz1[i][p] in[m][p], m over features and basis values;  the camera's sum of dz1 (lane = i)
      wave_lds_sync();
#pragma unroll
      for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int r = 0; r < 16; ++r) TA[(mt * 32 + drow(r, half)) * TS + j] = D1[mt][r];
      wave_lds_sync();
#pragma unroll 2
      for (int s = 0; s < 16; ++s) {
        const int p = 2 * s + half;
        const float a0 = TA[j * TS + p], a1 = TA[(32 + j) * TS + p], b0 = TI[j * TS + p], tq = TI[(FEAT + (j & 15)) * TS + p];
        const float b1 = j < NSH ? tq : 0.f;
        DW1[0] = mfma(a0, b0, DW1[0]); DW1[1] = mfma(a0, b1, DW1[1]); DW1[2] = mfma(a1, b0, DW1[2]); DW1[3] = mfma(a1, b1, DW1[3]);
      }
      {
        float sum = 0.f;
#pragma unroll
        for (int p = 0; p < 32; ++p) sum += TA[lane * TS + p];
        float* slot = part_s1 + (((size_t)blockIdx.x * 4 + wave) * a.C + c) * HID + lane;
        *slot = t == 0 ? sum : *slot + sum;
      }
    }
    if (valid) {
      float4* dst = (float4*)(v_features + (size_t)g * FEAT);
#pragma unroll
      for (int q = 0; q < 4; ++q) dst[2 * q + half] = make_float4(vf[4 * q], vf[4 * q + 1], vf[4 * q + 2], vf[4 * q + 3]);
    }
  }
  // the block's partial set: the waves add theirs in wave order into S (the transposes' LDS), then one copy to the workspace
  __syncthreads();
  float* const S = tbase;
  float* const R3 = tbase + P_SIZE;   // [4 waves][32 lanes][3]
  if (half == 0) { R3[(wave * 32 + j) * 3] = db3[0]; R3[(wave * 32 + j) * 3 + 1] = db3[1]; R3[(wave * 32 + j) * 3 + 2] = db3[2]; }
  for (int w = 0; w < 4; ++w) {
    if (wave == w) {
#pragma unroll
      for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int i = (q >> 1) * 32 + drow(r, half), col = (q & 1) * 32 + j;
          float* s2 = S + P_W2 + i * HID + col;
          *s2 = w == 0 ? DW2[q][r] : *s2 + DW2[q][r];
          if (col < FEAT + NSH) {
            float* s1 = S + P_W1 + i * (FEAT + NSH) + col;
            *s1 = w == 0 ? DW1[q][r] : *s1 + DW1[q][r];
          }
        }
#pragma unroll
      for (int o = 0; o < 3; ++o) {
        float* s3 = S + P_W3 + o * HID + lane;
        *s3 = w == 0 ? dw3[o] : *s3 + dw3[o];
      }
      float* sb = S + P_B2 + lane;
      *sb = w == 0 ? db2 : *sb + db2;
    }
    __syncthreads();
  }
  if (threadIdx.x < 4) {
    double sum = 0.0;   // 128 lane sums in lane order, added in fp64 and rounded once
    if (threadIdx.x < 3)
      for (int q = 0; q < 128; ++q) sum += (double)R3[3 * q + threadIdx.x];
    S[P_B3 + threadIdx.x] = (float)sum;
  }
  __syncthreads();
  for (int idx = threadIdx.x; idx < P_SIZE; idx += 256) part[(size_t)blockIdx.x * P_SIZE + idx] = S[idx];
}

// the fp32 partials are added in fp64 and rounded once (up to 512 x 4 of them: a running fp32 sum would lose several bits).
// red [P_SIZE] = the blocks' partial sets added in block order; s1 [C][64] = the (block, wave) slots of the per-camera sums in that order
__global__ __launch_bounds__(256) void appearance_reduce_kernel(const float* __restrict__ part, const float* __restrict__ part_s1, int blocks, int C,
                                                                float* __restrict__ red, float* __restrict__ s1) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e < P_SIZE) {
    double sum = 0.0;
    for (int b = 0; b < blocks; ++b) sum += (double)part[(size_t)b * P_SIZE + e];
    red[e] = (float)sum;
  } else if (e < P_SIZE + C * HID) {
    const int q = e - P_SIZE, c = q >> 6, i = q & 63;
    double sum = 0.0;
    for (int bw = 0; bw < blocks * 4; ++bw) sum += (double)part_s1[((size_t)bw * C + c) * HID + i];
    s1[q] = (float)sum;
  }
}

// the parameter gradients in the module's own layouts.  Thread e: [0, 64 in_dim) W1.grad, then b1 64, W2 4096, b2 64, W3 192, b3 3, then
// embeds.grad n_embeds x 16 (every element written: zeros for a row no camera names)
__global__ __launch_bounds__(256) void appearance_finalize_kernel(WmAppearanceArgs a, const float* __restrict__ red, const float* __restrict__ s1,
                                                                  float* __restrict__ v_W1, float* __restrict__ v_b1, float* __restrict__ v_W2,
                                                                  float* __restrict__ v_b2, float* __restrict__ v_W3, float* __restrict__ v_b3,
                                                                  float* __restrict__ v_embeds) {
  const int in_dim = EMB + FEAT + a.n_bases;
  long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e < HID * in_dim) {
    const int i = (int)e / in_dim, col = (int)e % in_dim;
    float v;
    if (col < EMB) {   // sum over cameras, in order, of (sum_g dz1[c])[i] embed[c][col]
      v = 0.f;
      for (int c = 0; c < a.C; ++c) {
        const float* em = embed_row(a, c);
        if (em) v = fmaf(s1[c * HID + i], em[col], v);
      }
    } else {
      v = red[P_W1 + i * (FEAT + NSH) + col - EMB];
    }
    v_W1[e] = v;
    return;
  }
  e -= HID * in_dim;
  if (e < HID) {
    double v = 0.0;
    for (int c = 0; c < a.C; ++c) v += (double)s1[c * HID + e];
    v_b1[e] = (float)v;
    return;
  }
  e -= HID;
  if (e < HID * HID) { v_W2[e] = red[P_W2 + e]; return; }
  e -= HID * HID;
  if (e < HID) { v_b2[e] = red[P_B2 + e]; return; }
  e -= HID;
  if (e < 3 * HID) { v_W3[e] = red[P_W3 + e]; return; }
  e -= 3 * HID;
  if (e < 3) { v_b3[e] = red[P_B3 + e]; return; }
  e -= 3;
  if (v_embeds && e < (long long)a.n_embeds * EMB) {
    const int row = (int)(e / EMB), k = (int)(e % EMB);
    float v = 0.f;
    if (a.embed_ids) {
      for (int c = 0; c < a.C; ++c) {
        if (a.embed_ids[c] != row) continue;
        float d = 0.f;
        for (int i = 0; i < HID; ++i) d = fmaf(a.W1[i * in_dim + k], s1[c * HID + i], d);
        v += d;
      }
    }
    v_embeds[e] = v;
  }
}

struct BwdPlan { int tiles, tiles_per_block, blocks; size_t part, part_s1, red, s1, total; };
BwdPlan plan_bwd(int N, int C) {
  BwdPlan p;
  p.tiles = (N + BLOCK_G - 1) / BLOCK_G;
  p.tiles_per_block = (p.tiles + MAX_BLOCKS - 1) / MAX_BLOCKS;
  p.blocks = (p.tiles + p.tiles_per_block - 1) / p.tiles_per_block;
  auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
  p.part = 0;
  p.part_s1 = p.part + al((size_t)p.blocks * P_SIZE * sizeof(float));
  p.red = p.part_s1 + al((size_t)p.blocks * 4 * C * HID * sizeof(float));
  p.s1 = p.red + al(P_SIZE * sizeof(float));
  p.total = p.s1 + al((size_t)C * HID * sizeof(float));
  return p;
}

bool args_valid(const WmAppearanceArgs& a) {
  return a.N > 0 && a.C > 0 && a.degree >= 0 && a.degree <= 3 && (a.n_bases == 1 || a.n_bases == 4 || a.n_bases == 9 || a.n_bases == 16) &&
         (a.degree + 1) * (a.degree + 1) <= a.n_bases && (size_t)a.N * a.C < (1ull << 29) && a.features && a.dirs && a.W1 && a.b1 && a.W2 && a.b2 &&
         a.W3 && a.b3 && (!a.embed_ids || (a.embeds && a.n_embeds > 0));
}

template <int L>
void launch_bwd(const WmAppearanceArgs& a, const BwdPlan& p, const float* v_out, float* v_features, float* v_dirs, float* part, float* part_s1,
                hipStream_t s) {
  constexpr size_t shm = (size_t)(W_FLOATS + 4 * T_WAVE) * sizeof(float);
  // on every launch: the attribute belongs to the current device, and a flag set once per process would leave a second device without it
  (void)hipFuncSetAttribute((const void*)appearance_bwd_kernel<L>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm);
  hipLaunchKernelGGL(appearance_bwd_kernel<L>, dim3((unsigned)p.blocks), dim3(256), shm, s, a, v_out, v_features, v_dirs, part, part_s1, p.tiles_per_block);
}

}  // namespace

size_t wm_appearance_bwd_workspace_bytes(int N, int C) { return N > 0 && C > 0 ? plan_bwd(N, C).total : 0; }

hipError_t wm_launch_appearance_fwd(const WmAppearanceArgs& a, float* out, hipStream_t s) {
  if (!args_valid(a) || !out) return hipErrorInvalidValue;
  const dim3 grid((unsigned)((a.N + BLOCK_G - 1) / BLOCK_G));
  if (a.degree == 0) hipLaunchKernelGGL(appearance_fwd_kernel<0>, grid, dim3(256), 0, s, a, out);
  else if (a.degree == 1) hipLaunchKernelGGL(appearance_fwd_kernel<1>, grid, dim3(256), 0, s, a, out);
  else if (a.degree == 2) hipLaunchKernelGGL(appearance_fwd_kernel<2>, grid, dim3(256), 0, s, a, out);
  else hipLaunchKernelGGL(appearance_fwd_kernel<3>, grid, dim3(256), 0, s, a, out);
  return hipGetLastError();
}

hipError_t wm_launch_appearance_bwd(const WmAppearanceArgs& a, const WmAppearanceGrads& v, void* ws, size_t ws_bytes, hipStream_t s) {
  if (!args_valid(a) || !v.v_out || !v.v_features || !v.v_dirs || !v.v_W1 || !v.v_b1 || !v.v_W2 || !v.v_b2 || !v.v_W3 || !v.v_b3 || !ws)
    return hipErrorInvalidValue;
  const BwdPlan p = plan_bwd(a.N, a.C);
  if (ws_bytes < p.total) return hipErrorInvalidValue;
  float* part = (float*)((char*)ws + p.part);
  float* part_s1 = (float*)((char*)ws + p.part_s1);
  float* red = (float*)((char*)ws + p.red);
  float* s1 = (float*)((char*)ws + p.s1);
  if (a.degree == 0) launch_bwd<0>(a, p, v.v_out, v.v_features, v.v_dirs, part, part_s1, s);
  else if (a.degree == 1) launch_bwd<1>(a, p, v.v_out, v.v_features, v.v_dirs, part, part_s1, s);
  else if (a.degree == 2) launch_bwd<2>(a, p, v.v_out, v.v_features, v.v_dirs, part, part_s1, s);
  else launch_bwd<3>(a, p, v.v_out, v.v_features, v.v_dirs, part, part_s1, s);
  hipLaunchKernelGGL(appearance_reduce_kernel, dim3((unsigned)((P_SIZE + a.C * HID + 255) / 256)), dim3(256), 0, s, part, part_s1, p.blocks, a.C, red, s1);
  const long long n_out = (long long)HID * (EMB + FEAT + a.n_bases) + HID + HID * HID + HID + 3 * HID + 3 + (v.v_embeds ? (long long)a.n_embeds * EMB : 0);
  hipLaunchKernelGGL(appearance_finalize_kernel, dim3((unsigned)((n_out + 255) / 256)), dim3(256), 0, s, a, red, s1, v.v_W1, v.v_b1, v.v_W2, v.v_b2, v.v_W3,
                     v.v_b3, v.v_embeds);
  return hipGetLastError();
}
