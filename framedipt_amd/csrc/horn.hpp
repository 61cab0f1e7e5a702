// horn.hpp — the superposition primitives evaluate.hip and tmscore.hip share: one Jacobi rotation of a symmetric 4 x 4 matrix and
// Horn's closed form (the unit quaternion of the best proper rotation is the eigenvector of the largest eigenvalue of a 4 x 4 matrix
// formed from the 3 x 3 covariance), solved by Jacobi sweeps in registers.  Plain float64 arithmetic in a fixed order: an including
// unit decides about contraction (#pragma clang fp contract) before it includes this file.
#pragma once

// one Jacobi rotation of the symmetric A that zeroes A[P][Q]; V collects the rotations (its columns become the eigenvectors)
template <int P, int Q>
__device__ __forceinline__ void fd_jacobi(double (&A)[4][4], double (&V)[4][4]) {
  const double apq = A[P][Q];
  if (apq == 0.0) return;
  const double theta = (A[Q][Q] - A[P][P]) / (2.0 * apq);
  const double t = copysign(1.0, theta) / (fabs(theta) + sqrt(theta * theta + 1.0));
  const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (k != P && k != Q) {
      const double akp = A[k][P], akq = A[k][Q];
      A[k][P] = A[P][k] = c * akp - s * akq;
      A[k][Q] = A[Q][k] = s * akp + c * akq;
    }
  }
  A[P][P] -= t * apq;
  A[Q][Q] += t * apq;
  A[P][Q] = A[Q][P] = 0.0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const double vkp = V[k][P], vkq = V[k][Q];
    V[k][P] = c * vkp - s * vkq;
    V[k][Q] = s * vkp + c * vkq;
  }
}

// H = sum (a - ca)(b - cb)' (row-major) -> R (row-major) with R a ~ b, no reflection.  `top` and `second` are the two largest
// eigenvalues of Horn's matrix (the first diagonal entry equal to `top` is the eigenvalue taken; a second one is a gap of 0), `scale`
// the sum of the absolute values of its entries: the rotation is unique where top - second is more than rounding of scale.
__device__ __forceinline__ void fd_horn_rotation(const double (&H)[9], double (&R)[9], double& top, double& second, double& scale) {
  double A[4][4] = {{H[0] + H[4] + H[8], H[5] - H[7], H[6] - H[2], H[1] - H[3]},
                    {H[5] - H[7], H[0] - H[4] - H[8], H[1] + H[3], H[6] + H[2]},
                    {H[6] - H[2], H[1] + H[3], H[4] - H[0] - H[8], H[5] + H[7]},
                    {H[1] - H[3], H[6] + H[2], H[5] + H[7], H[8] - H[0] - H[4]}};
  double V[4][4] = {{1.0, 0.0, 0.0, 0.0}, {0.0, 1.0, 0.0, 0.0}, {0.0, 0.0, 1.0, 0.0}, {0.0, 0.0, 0.0, 1.0}};
  scale = 0.0;
#pragma unroll
  for (int p = 0; p < 4; ++p)
#pragma unroll
    for (int q = 0; q < 4; ++q) scale += fabs(A[p][q]);
  for (int sweep = 0; sweep < 32; ++sweep) {
    const double off = fabs(A[0][1]) + fabs(A[0][2]) + fabs(A[0][3]) + fabs(A[1][2]) + fabs(A[1][3]) + fabs(A[2][3]);
    if (off <= 1e-22 * scale) break;
    fd_jacobi<0, 1>(A, V);
    fd_jacobi<0, 2>(A, V);
    fd_jacobi<0, 3>(A, V);
    fd_jacobi<1, 2>(A, V);
    fd_jacobi<1, 3>(A, V);
    fd_jacobi<2, 3>(A, V);
  }
  top = A[0][0];
  double q0 = V[0][0], q1 = V[1][0], q2 = V[2][0], q3 = V[3][0];
#pragma unroll
  for (int k = 1; k < 4; ++k)
    if (A[k][k] > top) { top = A[k][k]; q0 = V[0][k]; q1 = V[1][k]; q2 = V[2][k]; q3 = V[3][k]; }
  second = -1.0 / 0.0;
  bool seen = false;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (A[k][k] == top && !seen) seen = true;
    else second = fmax(second, A[k][k]);
  }
  const double qn = 1.0 / sqrt(q0 * q0 + q1 * q1 + q2 * q2 + q3 * q3);
  q0 *= qn; q1 *= qn; q2 *= qn; q3 *= qn;
  R[0] = q0 * q0 + q1 * q1 - q2 * q2 - q3 * q3; R[1] = 2.0 * (q1 * q2 - q0 * q3); R[2] = 2.0 * (q1 * q3 + q0 * q2);
  R[3] = 2.0 * (q1 * q2 + q0 * q3); R[4] = q0 * q0 - q1 * q1 + q2 * q2 - q3 * q3; R[5] = 2.0 * (q2 * q3 - q0 * q1);
  R[6] = 2.0 * (q1 * q3 - q0 * q2); R[7] = 2.0 * (q2 * q3 + q0 * q1); R[8] = q0 * q0 - q1 * q1 - q2 * q2 + q3 * q3;
}
