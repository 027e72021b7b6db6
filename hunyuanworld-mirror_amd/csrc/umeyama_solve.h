// The closed form of Umeyama's least-squares similarity (IEEE TPAMI 13(4), 1991) on finished moments, in fp64, for one thread: the 3 x 3
// singular value decomposition by one-sided Jacobi rotations (Hestenes), the determinant correction, scale, rotation and translation.
// Plain C++ so that a host program can run the same statements (tools and CPU builds include it without the HIP runtime).
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define UM_HD __host__ __device__ inline
#else
#define UM_HD inline
#endif

// A = U diag(sg) V^T, sg descending, U and V orthogonal (row-major 3 x 3).  The columns of A are rotated pairwise until they are orthogonal
// to 2^-52 of their lengths, which gives small singular values and their vectors to full relative accuracy; the columns then are U sg.  A
// column of length 0 (rank below 3) is completed by a cross product, or by Gram-Schmidt on a coordinate axis.
UM_HD void um_svd3(const double* A, double* U, double* sg, double* V) {
  double G[9], W[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
  double big = 0.0;
  for (int i = 0; i < 9; ++i) big = fmax(big, fabs(A[i]));
  const double pre = big > 0.0 ? 1.0 / big : 0.0;      // entries of size 1: no square under- or overflows
  for (int i = 0; i < 9; ++i) G[i] = A[i] * pre;
  for (int sweep = 0; sweep < 40; ++sweep) {
    bool moved = false;
    for (int p = 0; p < 2; ++p)
      for (int q = p + 1; q < 3; ++q) {
        double al = 0.0, be = 0.0, ga = 0.0;
        for (int r = 0; r < 3; ++r) { al += G[3 * r + p] * G[3 * r + p]; be += G[3 * r + q] * G[3 * r + q]; ga += G[3 * r + p] * G[3 * r + q]; }
        if (ga == 0.0 || fabs(ga) <= 2.220446049250313e-16 * sqrt(al * be)) continue;
        moved = true;
        const double zeta = (be - al) / (2.0 * ga);
        const double tt = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
        const double c = 1.0 / sqrt(1.0 + tt * tt), s = c * tt;
        for (int r = 0; r < 3; ++r) {
          const double gp = G[3 * r + p], gq = G[3 * r + q];
          G[3 * r + p] = c * gp - s * gq;
          G[3 * r + q] = s * gp + c * gq;
          const double wp = W[3 * r + p], wq = W[3 * r + q];
          W[3 * r + p] = c * wp - s * wq;
          W[3 * r + q] = s * wp + c * wq;
        }
      }
    if (!moved) break;
  }
  double n[3];
  int o[3] = {0, 1, 2};
  for (int j = 0; j < 3; ++j) n[j] = sqrt(G[j] * G[j] + G[3 + j] * G[3 + j] + G[6 + j] * G[6 + j]);
  for (int a = 0; a < 2; ++a)      // descending, stable
    for (int b = 0; b < 2 - a; ++b)
      if (n[o[b]] < n[o[b + 1]]) { const int t = o[b]; o[b] = o[b + 1]; o[b + 1] = t; }
  for (int j = 0; j < 3; ++j) {
    const int c = o[j];
    sg[j] = n[c] * big;
    for (int r = 0; r < 3; ++r) { V[3 * r + j] = W[3 * r + c]; U[3 * r + j] = n[c] > 0.0 ? G[3 * r + c] / n[c] : 0.0; }
  }
  if (!(n[o[0]] > 0.0)) { for (int i = 0; i < 9; ++i) U[i] = (i % 4 == 0) ? 1.0 : 0.0; return; }
  if (!(n[o[1]] > 0.0)) {      // rank 1: the second column from the coordinate axis least along the first
    int ax = 0;
    for (int r = 1; r < 3; ++r) if (fabs(U[3 * r]) < fabs(U[3 * ax])) ax = r;
    double v[3] = {0, 0, 0}, dot, len = 0.0;
    v[ax] = 1.0;
    dot = U[3 * ax];
    for (int r = 0; r < 3; ++r) { v[r] -= dot * U[3 * r]; len += v[r] * v[r]; }
    len = sqrt(len);
    for (int r = 0; r < 3; ++r) U[3 * r + 1] = v[r] / len;
  }
  // The third column is the cross product of the first two, with the sign of the rotated column where that has a length: the same vector
  // for a full-rank A, and a unit vector orthogonal to the others where the column is 0 or rounding noise (a planar cloud, three pairs).
  const double cr[3] = {U[3] * U[7] - U[6] * U[4], U[6] * U[1] - U[0] * U[7], U[0] * U[4] - U[3] * U[1]};
  const double sign = cr[0] * U[2] + cr[1] * U[5] + cr[2] * U[8] < 0.0 ? -1.0 : 1.0;
  const double len = sqrt(cr[0] * cr[0] + cr[1] * cr[1] + cr[2] * cr[2]);
  for (int r = 0; r < 3; ++r) U[3 * r + 2] = sign * cr[r] / len;
}

UM_HD double um_det3(const double* M) {
  return M[0] * (M[4] * M[8] - M[5] * M[7]) - M[1] * (M[3] * M[8] - M[5] * M[6]) + M[2] * (M[3] * M[7] - M[4] * M[6]);
}

// cov [3][3] = mean of (dst - mean_dst)(src - mean_src)^T, var_src = mean of |src - mean_src|^2  ->  out: s, R [9] row-major, t [3], the
// minimiser of sum |dst - (s R src + t)|^2 over rotations R (det R = +1: the last singular direction is mirrored when det U det V < 0)
UM_HD void um_solve(const double* cov, double var_src, const double* mean_src, const double* mean_dst, int with_scale, double* out) {
  double U[9], V[9], sg[3];
  um_svd3(cov, U, sg, V);
  const double d = um_det3(U) * um_det3(V) < 0.0 ? -1.0 : 1.0;
  double* R = out + 1;
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) R[3 * i + j] = U[3 * i] * V[3 * j] + U[3 * i + 1] * V[3 * j + 1] + d * U[3 * i + 2] * V[3 * j + 2];
  const double s = with_scale ? (sg[0] + sg[1] + d * sg[2]) / var_src : 1.0;
  out[0] = s;
  for (int i = 0; i < 3; ++i) out[10 + i] = mean_dst[i] - s * (R[3 * i] * mean_src[0] + R[3 * i + 1] * mean_src[1] + R[3 * i + 2] * mean_src[2]);
}
