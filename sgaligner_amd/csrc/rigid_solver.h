// The least-squares rigid fit that ransac.hip (ransac_hyp_kernel, ransac_step_kernel), icp.hip (icp_step_kernel) and ransac_geo.hip
// (geo_models_kernel) share: one definition, so that a fix to the convergence test reaches all four kernels.
//
// ONE TEXT DOES NOT MEAN ONE SET OF BITS.  ransac.hip is built with -ffp-contract=fast, icp.hip and ransac_geo.hip with -ffp-contract=off
// (_build.FILE_FLAGS).  The solver's explicit fma() calls are the same everywhere, but its plain `a * b - c * d` expressions contract to
// fused operations in ransac.hip and stay two roundings each in the other two files -- exactly as they did when every file held its own
// copy.  No contract of include/sgaligner_hip.h claims that the three files give the same bits for the same moments.
#pragma once
#include <math.h>

#include <hip/hip_runtime.h>

constexpr int RIGID_SWEEPS = 10;                   // at most this many cyclic Jacobi sweeps on the 4x4 quaternion matrix (it converges in 5-6)
constexpr double RIGID_CONVERGED = 1e-32;          // ... stopping once |off-diagonal|^2 <= this x |diagonal|^2: a function of the matrix alone

// Least-squares rigid transform (proper rotation) from moments taken about a pivot (ps, pr): S = [sum s' (3) | sum r' (3) | sum s' r'^T (9)],
// s' = s - ps, r' = r - pr, over n pairs.  Horn's unit quaternion: the eigenvector of the largest eigenvalue of the symmetric 4x4 matrix
// built from the centred cross-covariance, by cyclic Jacobi sweeps.  All array indices are compile-time constants
// after unrolling, so everything stays in registers.  Returns false (out untouched) when a result is not finite.
__host__ __device__ inline bool rigid_from_moments(double n, const double* S, const double* ps, const double* pr, double* out) {
    const double inv = 1.0 / n;
    double ms[3], mr[3], H[3][3];
#pragma unroll
    for (int a = 0; a < 3; ++a) { ms[a] = S[a] * inv; mr[a] = S[3 + a] * inv; }
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) H[a][b] = S[6 + 3 * a + b] - S[a] * mr[b];
    double A[4][4], V[4][4];
    A[0][0] = H[0][0] + H[1][1] + H[2][2];
    A[1][1] = H[0][0] - H[1][1] - H[2][2];
    A[2][2] = -H[0][0] + H[1][1] - H[2][2];
    A[3][3] = -H[0][0] - H[1][1] + H[2][2];
    A[0][1] = A[1][0] = H[1][2] - H[2][1];
    A[0][2] = A[2][0] = H[2][0] - H[0][2];
    A[0][3] = A[3][0] = H[0][1] - H[1][0];
    A[1][2] = A[2][1] = H[0][1] + H[1][0];
    A[1][3] = A[3][1] = H[2][0] + H[0][2];
    A[2][3] = A[3][2] = H[1][2] + H[2][1];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) V[i][j] = i == j ? 1.0 : 0.0;
#pragma unroll 1
    for (int sweep = 0; sweep < RIGID_SWEEPS; ++sweep) {
        double offd = 0.0, diag = 0.0;
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            diag = fma(A[p][p], A[p][p], diag);
#pragma unroll
            for (int q = p + 1; q < 4; ++q) offd = fma(A[p][q], A[p][q], offd);
        }
        if (offd <= RIGID_CONVERGED * diag) break;            // off-diagonal norm at rounding level of the diagonal's: nothing left to rotate
#pragma unroll
        for (int p = 0; p < 3; ++p) {
#pragma unroll
            for (int q = p + 1; q < 4; ++q) {
                const double apq = A[p][q];
                const bool rot = apq != 0.0;
                const double theta = (A[q][q] - A[p][p]) / (2.0 * (rot ? apq : 1.0));
                const double tt = (theta < 0.0 ? -1.0 : 1.0) / (fabs(theta) + sqrt(fma(theta, theta, 1.0)));     // |theta| huge: 1 / inf = 0
                const double t = rot ? tt : 0.0;
                const double c = 1.0 / sqrt(fma(t, t, 1.0)), s = t * c;
                A[p][p] -= t * apq;
                A[q][q] += t * apq;
                A[p][q] = A[q][p] = 0.0;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    if (k != p && k != q) {
                        const double akp = A[k][p], akq = A[k][q];
                        A[k][p] = A[p][k] = c * akp - s * akq;
                        A[k][q] = A[q][k] = s * akp + c * akq;
                    }
                    const double vkp = V[k][p], vkq = V[k][q];
                    V[k][p] = c * vkp - s * vkq;
                    V[k][q] = s * vkp + c * vkq;
                }
            }
        }
    }
    double lam = A[0][0], w = V[0][0], x = V[1][0], y = V[2][0], z = V[3][0];
#pragma unroll
    for (int i = 1; i < 4; ++i)
        if (A[i][i] > lam) { lam = A[i][i]; w = V[0][i]; x = V[1][i]; y = V[2][i]; z = V[3][i]; }
    const double qn = 1.0 / sqrt(w * w + x * x + y * y + z * z);
    w *= qn; x *= qn; y *= qn; z *= qn;
    double R[9];
    R[0] = w * w + x * x - y * y - z * z;
    R[1] = 2.0 * (x * y - w * z);
    R[2] = 2.0 * (x * z + w * y);
    R[3] = 2.0 * (x * y + w * z);
    R[4] = w * w - x * x + y * y - z * z;
    R[5] = 2.0 * (y * z - w * x);
    R[6] = 2.0 * (x * z - w * y);
    R[7] = 2.0 * (y * z + w * x);
    R[8] = w * w - x * x - y * y + z * z;
    double t[3];
    bool fin = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double cx = ps[0] + ms[0], cy = ps[1] + ms[1], cz = ps[2] + ms[2];
        t[a] = (pr[a] + mr[a]) - (R[3 * a] * cx + R[3 * a + 1] * cy + R[3 * a + 2] * cz);
        fin = fin && isfinite(t[a]);
    }
#pragma unroll
    for (int a = 0; a < 9; ++a) fin = fin && isfinite(R[a]);
    if (!fin) return false;
#pragma unroll
    for (int a = 0; a < 9; ++a) out[a] = R[a];
#pragma unroll
    for (int a = 0; a < 3; ++a) out[9 + a] = t[a];
    return true;
}
