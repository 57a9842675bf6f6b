// NCA loss of the EVA baseline over blocks of the anchors x anchors score matrix: sums, loss terms, coefficient block.
//
// Replaces reference NCALoss.forward, src/aligner/losses.py:161-173, and its autograd.  With s = Z1 Z2^T over the A anchor pairs
// (rows of the L2-normalised table, OverallNCALoss :186-198):
//     S_ij = exp(alpha (s_ij - ep)), i != j;  S_ii = 0        r_i = sum_j S_ij        c_j = sum_i S_ij
//     loss = mean_j log(1 + c_j) / alpha + mean_i log(1 + r_i) / alpha - beta mean_j log(1 + relu(s_jj))
//     dloss/ds_ij = S_ij / A (1 / (1 + c_j) + 1 / (1 + r_i)), i != j        dloss/ds_jj = -beta / A [s_jj > 0] / (1 + s_jj)
// The products (s = Z1 Z2^T, dZ1 = g Z2, dZ2 = g^T Z1) are the library's GEMMs (nca_ops.py); the kernels here run over a row block
// [h, A] of s that a GEMM has materialised -- 2 D flops per score against a few bytes, so the block costs little next to its products:
//   sga_nca_block_sums   S on the fly (the block keeps s), row sums r_i, diagonal scores, per-group column partials
//   sga_nca_loss         folds the partials to c_j, the three log terms, and the reciprocals 1 / (1 + r_i), 1 / (1 + c_j) for the coefficients
//   sga_nca_coef         g (in place, or beside a block the caller keeps) and its transpose (a 32 x 32 LDS tile turn): both gradient products then run without a transposed
//                        operand, whose GEMM route adds its K splits with atomics
// No floating-point atomic: every sum is folded in a fixed order -- fp32 inside a tile (256 columns of a row / 32 rows of a column), fp64
// across tiles, row groups and blocks -- so the loss and both gradients are bitwise repeatable.
#include "sga_common.h"

namespace {

constexpr int NCA_RG = 256;           // rows per column-partial group
constexpr int NCA_TILE = 32;          // rows of a column folded in fp32
constexpr int NCA_THREADS = 256;

__device__ __forceinline__ float nca_s(float s, float alpha, float ep) { return expf(alpha * (s - ep)); }

// one wave per row of the block: r_i and the diagonal score
__global__ __launch_bounds__(NCA_THREADS) void nca_row_kernel(const float* __restrict__ S, long lds, int h, int A, int row0, float alpha,
                                                              float ep, double* __restrict__ rsum, float* __restrict__ diag) {
    const int lane = threadIdx.x & 63, wpb = NCA_THREADS / 64;
    for (int r = blockIdx.x * wpb + (threadIdx.x >> 6); r < h; r += gridDim.x * wpb) {
        const float* s = S + (size_t)r * lds;
        const int gi = row0 + r;
        double acc = 0.0;
        for (int j0 = 0; j0 < A; j0 += 256) {
            float p = 0.f;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int j = j0 + lane + 64 * k;
                if (j < A && j != gi) p += nca_s(s[j], alpha, ep);
            }
            acc += (double)wave_sum(p);
        }
        if (lane == 0) { rsum[gi] = acc; diag[gi] = s[gi]; }
    }
}

// one thread per column and row group: the group's share of c_j
__global__ __launch_bounds__(NCA_THREADS) void nca_col_kernel(const float* __restrict__ S, long lds, int h, int A, int row0, float alpha,
                                                              float ep, double* __restrict__ cpart) {
    const int j = blockIdx.x * NCA_THREADS + threadIdx.x;
    if (j >= A) return;
    const int r0 = blockIdx.y * NCA_RG, r1 = min(h, r0 + NCA_RG);
    double acc = 0.0;
    for (int t0 = r0; t0 < r1; t0 += NCA_TILE) {
        float p = 0.f;
        const int t1 = min(r1, t0 + NCA_TILE);
        for (int r = t0; r < t1; ++r)
            if (row0 + r != j) p += nca_s(S[(size_t)r * lds + j], alpha, ep);
        acc += (double)p;
    }
    cpart[(size_t)blockIdx.y * A + j] = acc;
}

__global__ __launch_bounds__(NCA_THREADS) void nca_fold_kernel(const double* __restrict__ rsum, const double* __restrict__ cpart, int ngroups,
                                                               int A, double* __restrict__ csum, float* __restrict__ invr,
                                                               float* __restrict__ invc) {
    const int j = blockIdx.x * NCA_THREADS + threadIdx.x;
    if (j >= A) return;
    double c = 0.0;
    for (int g = 0; g < ngroups; ++g) c += cpart[(size_t)g * A + j];
    csum[j] = c;
    invc[j] = (float)(1.0 / (1.0 + c));
    invr[j] = (float)(1.0 / (1.0 + rsum[j]));
}

// one workgroup: the three log terms, strided per thread and folded through LDS in a fixed tree
__global__ __launch_bounds__(NCA_THREADS) void nca_loss_kernel(const double* __restrict__ rsum, const double* __restrict__ csum,
                                                               const float* __restrict__ diag, int A, double alpha, double beta,
                                                               double* __restrict__ loss) {
    __shared__ double red[3][NCA_THREADS];
    const int tid = threadIdx.x;
    double a = 0.0, b = 0.0, d = 0.0;
    for (int j = tid; j < A; j += NCA_THREADS) {
        a += log1p(csum[j]);
        b += log1p(rsum[j]);
        d += log1p(fmax((double)diag[j], 0.0));
    }
    red[0][tid] = a; red[1][tid] = b; red[2][tid] = d;
    __syncthreads();
    for (int o = NCA_THREADS / 2; o > 0; o >>= 1) {
        if (tid < o) { red[0][tid] += red[0][tid + o]; red[1][tid] += red[1][tid + o]; red[2][tid] += red[2][tid + o]; }
        __syncthreads();
    }
    if (tid == 0) loss[0] = red[0][0] / A / alpha + red[1][0] / A / alpha - beta * (red[2][0] / A);
}

// g = gout dloss/ds over a 32 x 32 tile of the block into Gm (in place when Gm == S), and transposed into GT [A, ldt]
__global__ __launch_bounds__(NCA_THREADS) void nca_coef_kernel(const float* S, long lds, float* Gm, long ldg, float* __restrict__ GT, long ldt, int h, int A,
                                                               int row0, float alpha, float beta, float ep, const float* __restrict__ invr,
                                                               const float* __restrict__ invc, const double* __restrict__ gout) {
    __shared__ float tile[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int j0 = blockIdx.x * 32, i0 = blockIdx.y * 32;
    const float sc = (float)gout[0] / (float)A;
    const int j = j0 + tx;
    const int h4 = min((long)((h + 3) & ~3), ldt);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int r = i0 + ty + 8 * k;
        float g = 0.f;
        if (r < h && j < A) {
            const int gi = row0 + r;
            const float s = S[(size_t)r * lds + j];
            if (gi == j) g = s > 0.f ? -beta * sc / (1.f + s) : 0.f;
            else g = nca_s(s, alpha, ep) * (invc[j] + invr[gi]) * sc;
            Gm[(size_t)r * ldg + j] = g;                                 // (Gm may be S itself: every element is read and written by one thread)
        }
        tile[ty + 8 * k][tx] = g;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int jj = j0 + ty + 8 * k, r = i0 + tx;
        if (jj < A && r < h4) GT[(size_t)jj * ldt + r] = tile[tx][ty + 8 * k];     // columns h .. h4 of GT: zeros (tile holds 0 there)
    }
}

int nca_check(const void* S, long lds, int h, int A, int row0, const char* who) {
    if (A < 1 || h < 1 || row0 < 0 || (long)row0 + h > A) {
        sga_set_error("%s: row block [%d, %d + %d) outside the %d anchors", who, row0, row0, h, A);
        return SGA_ERR_ARG;
    }
    if (lds < A) { sga_set_error("%s: leading dimension %ld < A = %d", who, lds, A); return SGA_ERR_ARG; }
    if (!S) { sga_set_error("%s: null pointer", who); return SGA_ERR_ARG; }
    return SGA_OK;
}

}  // namespace

extern "C" int sga_nca_row_group(void) { return NCA_RG; }

extern "C" int sga_nca_block_sums(const float* S, long lds, int h, int A, int row0, float alpha, float ep, double* rsum, float* diag,
                                  double* cpart, void* stream) {
    const int rc = nca_check(S, lds, h, A, row0, "sga_nca_block_sums");
    if (rc) return rc;
    SGA_CHECK_ARG(rsum && diag && cpart, "sga_nca_block_sums: null pointer");
    hipStream_t s = static_cast<hipStream_t>(stream);
    int g = (h + 3) / 4;
    const int cap = sga_num_cus() * 8;
    if (g > cap) g = cap;
    hipLaunchKernelGGL(nca_row_kernel, dim3(g), dim3(NCA_THREADS), 0, s, S, lds, h, A, row0, alpha, ep, rsum, diag);
    hipLaunchKernelGGL(nca_col_kernel, dim3((A + NCA_THREADS - 1) / NCA_THREADS, (h + NCA_RG - 1) / NCA_RG), dim3(NCA_THREADS), 0, s, S, lds,
                       h, A, row0, alpha, ep, cpart);
    SGA_CHECK_LAUNCH("sga_nca_block_sums");
    return SGA_OK;
}

extern "C" int sga_nca_loss(const double* rsum, const double* cpart, int ngroups, const float* diag, int A, float alpha, float beta,
                            double* csum, float* invr, float* invc, double* loss, void* stream) {
    SGA_CHECK_ARG(A >= 1 && ngroups >= 1, "sga_nca_loss: A = %d, %d row groups: both must be >= 1", A, ngroups);
    SGA_CHECK_ARG(alpha > 0.f, "sga_nca_loss: alpha must be positive");
    SGA_CHECK_ARG(rsum && cpart && diag && csum && invr && invc && loss, "sga_nca_loss: null pointer");
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(nca_fold_kernel, dim3((A + NCA_THREADS - 1) / NCA_THREADS), dim3(NCA_THREADS), 0, s, rsum, cpart, ngroups, A, csum,
                       invr, invc);
    hipLaunchKernelGGL(nca_loss_kernel, dim3(1), dim3(NCA_THREADS), 0, s, rsum, csum, diag, A, (double)alpha, (double)beta, loss);
    SGA_CHECK_LAUNCH("sga_nca_loss");
    return SGA_OK;
}

extern "C" int sga_nca_coef(const float* S, long lds, float* G, long ldg, float* GT, long ldt, int h, int A, int row0, float alpha,
                            float beta, float ep, const float* invr, const float* invc, const double* gout, void* stream) {
    const int rc = nca_check(S, lds, h, A, row0, "sga_nca_coef");
    if (rc) return rc;
    SGA_CHECK_ARG(G && ldg >= A && (G != S || ldg == lds), "sga_nca_coef: bad coefficient block (null, leading dimension %ld < A = %d, or in place with another leading dimension)", ldg, A);
    SGA_CHECK_ARG(ldt >= h, "sga_nca_coef: leading dimension %ld of the transposed block < h = %d", ldt, h);
    SGA_CHECK_ARG(GT && invr && invc && gout, "sga_nca_coef: null pointer");
    hipLaunchKernelGGL(nca_coef_kernel, dim3((A + 31) / 32, (h + 31) / 32), dim3(NCA_THREADS), 0, static_cast<hipStream_t>(stream), S, lds,
                       G, ldg, GT, ldt, h, A, row0, alpha, beta, ep, invr, invc, gout);
    SGA_CHECK_LAUNCH("sga_nca_coef");
    return SGA_OK;
}
