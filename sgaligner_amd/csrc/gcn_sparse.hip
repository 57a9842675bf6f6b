// GCN aggregation over the compressed edge list of gat_sparse.hip (CSR): the route of MultiGCN for graphs of ANY size, fwd + bwd, no atomics.
//
// gcn.hip keeps one graph's N x N multiplicity matrix in LDS (at most 256 nodes per graph, 255 copies of a pair) and rebuilds it from the
// edge list in every launch.  Here the structure the sparse GAT route builds once per batch (GraphBatch.sparse(): row_ptr / src / mult
// target-major, col_ptr / tgt / perm its transpose, batch-global node ids, ascending neighbours, 32-bit multiplicities, input self loops and
// out-of-range endpoints dropped, one self loop per node) carries the arithmetic of gcn.hip's header:
//     deg_i  = sum of mult over the target-major row of i (the added self loop counts 1)      dinv_i = (float)(1 / sqrt((double)deg_i))
//     coef_e = (float)mult_e * (dinv_out * dinv_nbr)                                            two separately rounded multiplies
//     forward     out[i] = sum_{entries e of row i} coef_e H[src_e] + bias (+ ReLU)             over row_ptr / src / mult
//     transpose   out[j] = sum_{entries e of column j} coef_e H[tgt_e]                          over col_ptr / tgt, mult read as mult[perm[e]]
// One kernel serves both directions by the choice of arrays.  A wave owns one (output row, slab of 256 channels): its lanes load up to 64
// entries (neighbour id, multiplicity, the neighbour's dinv) coalesced and form the coefficients, which are then broadcast lane by lane
// (v_readlane) while the lanes span the channels, four per lane; a feature row is read as one coalesced row.  Every output element is ONE
// lane's fmaf chain from 0 in ascending neighbour order, the bias added after the chain, then the ReLU -- exactly the chain of
// gcn_aggregate_kernel over its LDS row, so for a graph the dense route can take the two routes return the same bits.  The chain is never
// split: memory-level parallelism comes from issuing the row loads of GCN_SP_AHEAD entries before their fmas.  A long row is walked by its
// one wave.  No floating-point atomics: the output is a pure function of the input.
#include "sga_common.h"

namespace {

constexpr int GCN_SP_THREADS = 256;
constexpr int GCN_SP_WAVES = GCN_SP_THREADS / 64;
constexpr int GCN_SP_CK = 4;                                  // channel slots per lane: 256 channels per slab, as gcn.hip
constexpr int GCN_SP_AHEAD = 4;                               // entries whose feature rows are in flight before the first of their fmas
constexpr long long GCN_SP_CAP_MAX = 0x7fffffffLL - 64;       // entries: the 64-entry chunk loops' `b += 64` cannot pass 2^31

__device__ __forceinline__ int gsp_lane_i(int v, int k) { return __builtin_amdgcn_readlane(v, k); }
__device__ __forceinline__ float gsp_lane_f(float v, int k) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), k)); }

// one wave per node: the integer degree (order-free, exact), then the correctly rounded fp32 value of deg^-1/2 -- gcn.hip's expression
__global__ __launch_bounds__(GCN_SP_THREADS) void gcn_sp_dinv_kernel(const int* __restrict__ row_ptr, const int* __restrict__ mult, int T,
                                                                     float* __restrict__ dinv) {
    const int lane = threadIdx.x & 63;
    const long long w = (long long)blockIdx.x * GCN_SP_WAVES + (threadIdx.x >> 6);
    if (w >= T) return;
    const int beg = __builtin_amdgcn_readfirstlane(row_ptr[w]), end = __builtin_amdgcn_readfirstlane(row_ptr[w + 1]);
    int deg = 0;
    for (int b = beg; b < end; b += 64)
        if (b + lane < end) deg += mult[b + lane];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) deg += __shfl_xor(deg, o, 64);
    if (lane == 0) dinv[w] = (float)(1.0 / sqrt((double)deg));
}

// CJ live channel slots per lane (channel cbase + lane + 64 q); a lane past C reads channel C - 1 again and stores nothing
template <int CJ>
__global__ __launch_bounds__(GCN_SP_THREADS) void gcn_sp_aggregate_kernel(const float* __restrict__ H, const float* __restrict__ bias,
                                                                          const int* __restrict__ ptr, const int* __restrict__ nbr,
                                                                          const int* __restrict__ mult, const int* __restrict__ perm,
                                                                          const float* __restrict__ dinv, float* __restrict__ out, int T,
                                                                          int C, int relu) {
    const int lane = threadIdx.x & 63, cbase = blockIdx.y * (64 * GCN_SP_CK);
    const long long w = (long long)blockIdx.x * GCN_SP_WAVES + (threadIdx.x >> 6);
    if (w >= T) return;
    const int i = (int)w;
    const int beg = __builtin_amdgcn_readfirstlane(ptr[i]), end = __builtin_amdgcn_readfirstlane(ptr[i + 1]);
    const float di = dinv[i];
    int cc[CJ];
    bool cv[CJ];
    float acc[CJ];
#pragma unroll
    for (int q = 0; q < CJ; ++q) {
        const int c = cbase + lane + 64 * q;
        cv[q] = c < C;
        cc[q] = min(c, C - 1);
        acc[q] = 0.f;
    }
    for (int b = beg; b < end; b += 64) {
        const int u = b + lane, cnt = min(64, end - b);
        int j = 0;
        float coef = 0.f;
        if (u < end) {
            j = nbr[u];
            const int m = perm ? mult[perm[u]] : mult[u];
            coef = (float)m * (di * dinv[j]);
        }
        int k = 0;
        for (; k + GCN_SP_AHEAD <= cnt; k += GCN_SP_AHEAD) {
            float v[GCN_SP_AHEAD][CJ];
#pragma unroll
            for (int a = 0; a < GCN_SP_AHEAD; ++a) {
                const float* row = H + (size_t)gsp_lane_i(j, k + a) * C;
#pragma unroll
                for (int q = 0; q < CJ; ++q) v[a][q] = row[cc[q]];
            }
#pragma unroll
            for (int a = 0; a < GCN_SP_AHEAD; ++a) {
                const float ck = gsp_lane_f(coef, k + a);
#pragma unroll
                for (int q = 0; q < CJ; ++q) acc[q] = fmaf(ck, v[a][q], acc[q]);
            }
        }
        for (; k < cnt; ++k) {
            const float ck = gsp_lane_f(coef, k);
            const float* row = H + (size_t)gsp_lane_i(j, k) * C;
#pragma unroll
            for (int q = 0; q < CJ; ++q) acc[q] = fmaf(ck, row[cc[q]], acc[q]);
        }
    }
    float* o = out + (size_t)i * C;
#pragma unroll
    for (int q = 0; q < CJ; ++q)
        if (cv[q]) {
            const float v = acc[q] + (bias ? bias[cc[q]] : 0.f);
            o[cc[q]] = relu ? fmaxf(v, 0.f) : v;
        }
}

inline unsigned gsp_wave_blocks(int T) { return (unsigned)(((long long)T + GCN_SP_WAVES - 1) / GCN_SP_WAVES); }

}  // namespace

extern "C" int sga_gcn_sp_dinv(const int32_t* row_ptr, const int32_t* mult, int T, int cap, float* dinv, void* stream) {
    SGA_CHECK_ARG(T >= 0 && cap >= 0, "sga_gcn_sp_dinv: negative size");
    SGA_CHECK_ARG(cap <= GCN_SP_CAP_MAX, "sga_gcn_sp_dinv: capacity %d: must stay below 2^31 - 64", cap);
    SGA_CHECK_ARG(T <= cap, "sga_gcn_sp_dinv: capacity %d below the %d self loops", cap, T);
    if (T == 0) return SGA_OK;
    SGA_CHECK_ARG(row_ptr && mult && dinv, "sga_gcn_sp_dinv: null pointer");
    hipLaunchKernelGGL(gcn_sp_dinv_kernel, dim3(gsp_wave_blocks(T)), dim3(GCN_SP_THREADS), 0, static_cast<hipStream_t>(stream), row_ptr, mult, T,
                       dinv);
    SGA_CHECK_LAUNCH("sga_gcn_sp_dinv");
    return SGA_OK;
}

extern "C" int sga_gcn_sp_aggregate(const float* H, int C, const float* bias, const int32_t* ptr, const int32_t* nbr, const int32_t* mult,
                                    const int32_t* perm, const float* dinv, int T, int cap, int relu, float* out, void* stream) {
    SGA_CHECK_ARG(T >= 0 && cap >= 0, "sga_gcn_sp_aggregate: negative size");
    SGA_CHECK_ARG(C >= 1, "sga_gcn_sp_aggregate: width %d < 1", C);
    SGA_CHECK_ARG(cap <= GCN_SP_CAP_MAX, "sga_gcn_sp_aggregate: capacity %d: must stay below 2^31 - 64", cap);
    SGA_CHECK_ARG(T <= cap, "sga_gcn_sp_aggregate: capacity %d below the %d self loops", cap, T);
    SGA_CHECK_ARG(!perm || (!bias && !relu), "sga_gcn_sp_aggregate: the transposed direction (perm given) takes no bias and no ReLU");
    if (T == 0) return SGA_OK;
    SGA_CHECK_ARG(H && ptr && nbr && mult && dinv && out && H != out, "sga_gcn_sp_aggregate: null pointer (or out aliases H)");
    const dim3 grid(gsp_wave_blocks(T), (C + 64 * GCN_SP_CK - 1) / (64 * GCN_SP_CK)), block(GCN_SP_THREADS);
    hipStream_t s = static_cast<hipStream_t>(stream);
    switch (C > 64 * GCN_SP_CK ? GCN_SP_CK : (C + 63) / 64) {      // more than one slab: every slab runs all four slots, the last one masked
        case 1: hipLaunchKernelGGL(gcn_sp_aggregate_kernel<1>, grid, block, 0, s, H, bias, ptr, nbr, mult, perm, dinv, out, T, C, relu ? 1 : 0); break;
        case 2: hipLaunchKernelGGL(gcn_sp_aggregate_kernel<2>, grid, block, 0, s, H, bias, ptr, nbr, mult, perm, dinv, out, T, C, relu ? 1 : 0); break;
        case 3: hipLaunchKernelGGL(gcn_sp_aggregate_kernel<3>, grid, block, 0, s, H, bias, ptr, nbr, mult, perm, dinv, out, T, C, relu ? 1 : 0); break;
        default: hipLaunchKernelGGL(gcn_sp_aggregate_kernel<4>, grid, block, 0, s, H, bias, ptr, nbr, mult, perm, dinv, out, T, C, relu ? 1 : 0); break;
    }
    SGA_CHECK_LAUNCH("sga_gcn_sp_aggregate");
    return SGA_OK;
}
