// GCN structure encoder of the EVA baseline: symmetric-normalised neighbourhood sums over each scene graph's edge list, fwd + bwd.
//
// Replaces torch_geometric.nn.GCNConv (PyG 2.2.0, cached=False, every other argument at its default) as reference
// src/aligner/networks/gat.py:6-25 (MultiGCN) stacks it, driven per graph from src/aligner/eva.py:44-72:
//     h = x W^T                                                     (no bias in the linear; W [out, in])
//     edges: input self loops removed, one self loop of weight 1 added per node, duplicates keep multiplicity
//     deg_i = 1 + #{listed edges j -> i, j != i}                    dinv_i = deg_i^-1/2
//     out[i] = sum_{j -> i} dinv_j dinv_i h[j] + bias               (the self loop included: A^ = D^-1/2 (A + I) D^-1/2)
// The dense products (x W^T, dW, dx) run on the MFMA GEMM over ALL nodes of the batch at once; this file holds A^.  One kernel serves
// out = A^ h + b (+ ReLU) and dh = A^T d_out: the edge list is scattered once into an LDS multiplicity matrix cnt[row][col] (8-bit, integer
// LDS atomics -- row = target, col = source, swapped for the transpose), the in-degrees into an LDS counter per node, and a wave then owns
// one output row: it walks that row's multiplicities four at a time (wave-uniform words, empty words skipped) while its lanes span the
// channels, so every output element is ONE lane's fma chain in ascending source order -- no floating-point atomic anywhere, the output is a
// pure function of the input.  All 2B graphs of a batch go in ONE launch per layer and direction; feature rows are read from global memory
// (L2-resident: at most 256 x 400 floats per graph).  Widths are free (the reference's are 200 and 400): 256 channels per workgroup.
#include "sga_common.h"

namespace {

constexpr int GCN_MAXN = 256;         // nodes per graph (the multiplicity matrix and the per-node scalars fit 66 KiB of LDS)
constexpr int GCN_THREADS = 256;
constexpr int GCN_CK = 4;             // channels per lane: 256 channels per workgroup

inline size_t gcn_lds_bytes(int nmax) {
    const int npad = (nmax + 3) & ~3;
    return sizeof(int) * 2 * GCN_MAXN + (size_t)nmax * npad;
}

__global__ __launch_bounds__(GCN_THREADS) void gcn_aggregate_kernel(
    const float* __restrict__ H, const float* __restrict__ bias, const long long* __restrict__ edges, const int* __restrict__ node_off,
    const int* __restrict__ edge_off, float* __restrict__ out, int C, int nmax, int transpose, int relu, int* __restrict__ status) {
    extern __shared__ __attribute__((aligned(16))) unsigned gcn_lds[];
    int* deg = reinterpret_cast<int*>(gcn_lds);                       // [GCN_MAXN] in-degree with the self loop
    float* dinv = reinterpret_cast<float*>(gcn_lds + GCN_MAXN);      // [GCN_MAXN] deg^-1/2
    unsigned* cnt = gcn_lds + 2 * GCN_MAXN;                           // [N][npad / 4] packed u8 multiplicities
    const int g = blockIdx.x, cbase = blockIdx.y * (64 * GCN_CK);
    const int n0 = node_off[g], N = node_off[g + 1] - n0, e0 = edge_off[g], E = edge_off[g + 1] - e0;
    const int npad = (nmax + 3) & ~3, nw = npad >> 2;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (N <= 0 || N > nmax) return;
    for (int e = tid; e < N * nw; e += GCN_THREADS) cnt[e] = 0u;
    for (int i = tid; i < GCN_MAXN; i += GCN_THREADS) deg[i] = 1;     // the one self loop every node gets
    __syncthreads();
    // edge list -> multiplicities and in-degrees (self loops dropped, out-of-range ids ignored, counts saturate at 255: reported through `status`)
    for (int e = tid; e < E; e += GCN_THREADS) {
        const long long sj = edges[(size_t)(e0 + e) * 2 + 0], di = edges[(size_t)(e0 + e) * 2 + 1];
        if (sj != di && sj >= 0 && sj < N && di >= 0 && di < N) {
            const int idx = transpose ? (int)sj * npad + (int)di : (int)di * npad + (int)sj;
            const unsigned sh = 8u * (idx & 3);
            const unsigned old = atomicAdd(&cnt[idx >> 2], 1u << sh);
            if (((old >> sh) & 255u) == 255u) {
                atomicSub(&cnt[idx >> 2], 1u << sh);
                if (status) atomicOr(status, 1);                      // a (source, target) pair listed > 255 times: PyG would count them all
            } else {
                atomicAdd(&deg[(int)di], 1);
            }
        }
    }
    __syncthreads();
    unsigned char* cb = reinterpret_cast<unsigned char*>(cnt);
    for (int i = tid; i < N; i += GCN_THREADS) {
        cb[i * npad + i] = 1;
        // the correctly rounded fp32 value of deg^-1/2: IEEE fp64 square root and division, then one rounding (no approximate rsqrt)
        dinv[i] = (float)(1.0 / sqrt((double)deg[i]));
    }
    __syncthreads();
    bool cv[GCN_CK];
    float bv[GCN_CK];
#pragma unroll
    for (int k = 0; k < GCN_CK; ++k) {
        const int c = cbase + lane + 64 * k;
        cv[k] = c < C;
        bv[k] = (cv[k] && bias) ? bias[c] : 0.f;
    }
    const float* Hg = H + (size_t)n0 * C + cbase + lane;
    for (int i = wave; i < N; i += GCN_THREADS / 64) {
        const float di = dinv[i];
        float acc[GCN_CK];
#pragma unroll
        for (int k = 0; k < GCN_CK; ++k) acc[k] = 0.f;
        for (int w = 0; w < nw; ++w) {
            const unsigned word = __builtin_amdgcn_readfirstlane(cnt[i * nw + w]);
            if (word == 0u) continue;
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const unsigned m = (word >> (8 * b)) & 255u;
                if (m == 0u) continue;
                const int j = 4 * w + b;
                const float coef = (float)m * (di * dinv[j]);
                const float* row = Hg + (size_t)j * C;
#pragma unroll
                for (int k = 0; k < GCN_CK; ++k)
                    if (cv[k]) acc[k] = fmaf(coef, row[64 * k], acc[k]);
            }
        }
        float* o = out + (size_t)(n0 + i) * C + cbase + lane;
#pragma unroll
        for (int k = 0; k < GCN_CK; ++k)
            if (cv[k]) {
                const float v = acc[k] + bv[k];
                o[64 * k] = relu ? fmaxf(v, 0.f) : v;
            }
    }
}

// d_pre = d_y [y > 0] for y = relu(pre) (ReLU' = 0 at 0, as autograd defines it)
__global__ void relu_bwd_kernel(const float* __restrict__ y, const float* __restrict__ gy, float* __restrict__ gx, size_t n) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        gx[i] = y[i] > 0.f ? gy[i] : 0.f;
}

}  // namespace

extern "C" int sga_gcn_aggregate(const float* H, int C, const float* bias, const int64_t* edges, const int32_t* node_off,
                                 const int32_t* edge_off, int G, int nmax, int transpose, int relu, float* out, int32_t* status,
                                 void* stream) {
    SGA_CHECK_ARG(G >= 0 && nmax >= 0, "sga_gcn_aggregate: negative size");
    SGA_CHECK_ARG(C >= 1, "sga_gcn_aggregate: width %d < 1", C);
    SGA_CHECK_ARG(nmax <= GCN_MAXN, "sga_gcn_aggregate: a graph has %d nodes; the GCN kernels support at most %d per graph", nmax, GCN_MAXN);
    if (G == 0 || nmax == 0) return SGA_OK;
    SGA_CHECK_ARG(H && node_off && edge_off && out && H != out, "sga_gcn_aggregate: null pointer (or out aliases H)");
    const size_t lds = gcn_lds_bytes(nmax);
    auto k = gcn_aggregate_kernel;
    hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(k, dim3(G, (C + 64 * GCN_CK - 1) / (64 * GCN_CK)), dim3(GCN_THREADS), lds, static_cast<hipStream_t>(stream), H, bias,
                       reinterpret_cast<const long long*>(edges), node_off, edge_off, out, C, nmax, transpose ? 1 : 0, relu ? 1 : 0, status);
    SGA_CHECK_LAUNCH("sga_gcn_aggregate");
    return SGA_OK;
}

extern "C" int sga_relu_bwd(const float* y, const float* gy, float* gx, size_t n, void* stream) {
    if (n == 0) return SGA_OK;
    SGA_CHECK_ARG(y && gy && gx, "sga_relu_bwd: null pointer");
    size_t g = (n + 255) / 256; if (g > 8192) g = 8192;
    hipLaunchKernelGGL(relu_bwd_kernel, dim3((unsigned)g), dim3(256), 0, static_cast<hipStream_t>(stream), y, gy, gx, n);
    SGA_CHECK_LAUNCH("sga_relu_bwd");
    return SGA_OK;
}
