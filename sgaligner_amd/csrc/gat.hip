// GAT structure encoder: attention softmax-aggregate over each scene graph's edge list, fwd + bwd.
//
// Replaces torch_geometric.nn.GATConv (PyG 2.2.0; un-vendored dependency, req.yml:259) as it is used by
// reference src/aligner/networks/gat.py:36-37,44 (GATConv(in, 128, heads=2), defaults concat=True,
// negative_slope=0.2, add_self_loops=True, bias=True) driven per graph from sg_aligner.py:86-110:
//     h = x W^T ;  a_s[j] = <h[j], att_src>, a_d[i] = <h[i], att_dst>           (per head)
//     edges: input self loops removed, one self loop added per node, duplicates keep multiplicity
//     e_ij = leaky_relu(a_s[j] + a_d[i], 0.2);  alpha_ij = softmax over incoming j (max-subtracted, +1e-16)
//     out[i] = sum_j alpha_ij h[j] + bias
// The dense projections (x W^T and their gradients) run on the generic MFMA GEMM over ALL nodes of the
// batch at once; this file holds the per-graph part.  One workgroup per (graph, head): the head's
// projected features [N,128] live in LDS (row stride 129 -> conflict-free both along and across rows),
// the edge list is scattered once into an LDS multiplicity matrix cnt[i][j] (8-bit, LDS atomics), and
// the per-target softmax is a wavefront job: lanes span the sources j, max / sum by wave shuffles,
// alpha broadcast by v_readlane for the aggregate.  All 2B graphs of a batch go in ONE launch
// (the reference issues 2B sequential GATConv calls).  Graph traffic is byte-bound: 16 B/edge (int64
// pairs, read once per head) + 512 B/node/head in, 512 B/node/head out.
//
// Two kernel families, one pair of entry points (sga_gat_attn_fwd_hc / _bwd_hc).  First in the file, and described above, the kernels of
// 2 heads x 128 channels -- the reference model's layers -- with those two numbers literal; further down the general ones (any head count,
// 1 .. 256 channels, both run-time values).  The entry points launch the first family at exactly 2 x 128 and the second everywhere else.
#include "sga_common.h"

namespace {

constexpr int GAT_C = 128;            // channels per head (hidden_units[1:], sg_aligner.py:38)
constexpr int GAT_H = 2;              // heads
constexpr int GAT_HS = GAT_C + 1;     // LDS row stride
constexpr int GAT_MAXN = 128;         // nodes per graph with the features resident in LDS (NJ = 2 sources per lane)
constexpr int GAT_MAXN_BIG = 256;     // nodes per graph of the big-graph variant (NJ = 4, features read from global/L2)
constexpr int GAT_THREADS = 256;
constexpr int GAT_TB = 8;             // targets (fwd) / sources (bwd) a wave processes together: LDS reads per FMA / 8
constexpr float GAT_SLOPE = 0.2f;

// The kernels of 2 heads x 128 channels, the reference model's layers; sga_gat_attn_fwd_hc / _bwd_hc launch them at that shape (they measured
// faster there than the general kernels below, also with the width fixed at compile time: profiles/gat_unify_bench.json).
// Two instantiations of every kernel: <NJ = 2, LDSF = true> for graphs of up to 128 nodes (every real 3RScan sub-scan:
// the head's features [N,128] live in LDS) and <NJ = 4, LDSF = false> for up to 256 nodes, where only the multiplicity
// matrix and the per-node scalars stay in LDS and feature rows are read from global memory (L2-resident: 128 KiB per
// graph and head).  NJ = source slots per lane (source j = lane + 64 k).
struct GatLds {
    float* hs;      // [N][129]   (LDSF)
    float* dos;     // [N][129]   (LDSF, bwd only)
    float* as;      // [maxn]
    float* ad;      // [maxn]
    float* mx;      // [maxn]  row max     (bwd)
    float* den;     // [maxn]  row denom   (bwd)
    float* das;     // [maxn]  d a_s       (bwd)
    float* dad;     // [maxn]  d a_d       (bwd)
    unsigned* cnt;  // [N][npad/4] packed u8 multiplicities
};

template <int NJ, bool LDSF>
__device__ __forceinline__ GatLds carve(float* base, int nmax, bool bwd) {
    constexpr int MAXN = NJ * 64;
    GatLds l;
    float* p = base;
    l.hs = p; if (LDSF) p += nmax * GAT_HS;
    l.dos = p; if (LDSF && bwd) p += nmax * GAT_HS;
    l.as = p; p += MAXN;
    l.ad = p; p += MAXN;
    l.mx = p; p += MAXN;
    l.den = p; p += MAXN;
    l.das = p; p += MAXN;
    l.dad = p; p += MAXN;
    l.cnt = reinterpret_cast<unsigned*>(p);
    return l;
}

inline size_t gat_lds_bytes(int nmax, bool bwd, int nj, bool ldsf) {
    const int npad = (nmax + 3) & ~3;
    return sizeof(float) * ((ldsf ? (size_t)nmax * GAT_HS * (bwd ? 2 : 1) : 0) + 6 * (size_t)nj * 64) + (size_t)nmax * npad;
}

__device__ __forceinline__ float lrelu(float v) { return v > 0.f ? v : GAT_SLOPE * v; }

// feature rows of this (graph, head): LDS copy (stride 129) or the global rows themselves (stride heads * 128)
struct Rows { const float* p; int stride; };

// common prologue: load this head's features (LDSF), attention logits' node parts, multiplicity matrix
template <int NJ, bool LDSF>
__device__ __forceinline__ Rows gat_prologue(const GatLds& l, const float* __restrict__ H, const float* __restrict__ att_s,
                                             const float* __restrict__ att_d, const long long* __restrict__ edges,
                                             int n0, int N, int e0, int E, int hd, int npad, int* status = nullptr,
                                             bool complete = false) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* Hg = H + (size_t)n0 * (GAT_H * GAT_C) + hd * GAT_C;
    if (LDSF)
        for (int e = tid; e < N * GAT_C; e += GAT_THREADS) {
            const int j = e >> 7, c = e & 127;
            l.hs[j * GAT_HS + c] = Hg[(size_t)j * (GAT_H * GAT_C) + c];
        }
    // COMPLETE graph (every ordered pair i != j listed exactly once: what preprocessing/scan3r/preprocess.py:176-182 writes for every
    // scene, verified per batch by gat_complete_kernel): with the self loops GATConv adds, every multiplicity is 1 -- the 16-byte-per-edge
    // list (2.13 GB at configs[2], read by 8 workgroup sets per step) is never touched.
    if (complete) {
        for (int e = tid; e < N * (npad >> 2); e += GAT_THREADS) {
            const int j4 = (e % (npad >> 2)) * 4;
            l.cnt[e] = (j4 + 0 < N ? 1u : 0u) | (j4 + 1 < N ? 0x100u : 0u) | (j4 + 2 < N ? 0x10000u : 0u) | (j4 + 3 < N ? 0x1000000u : 0u);
        }
    } else {
        for (int e = tid; e < N * (npad >> 2); e += GAT_THREADS) l.cnt[e] = 0u;
    }
    __syncthreads();
    const Rows hr = LDSF ? Rows{l.hs, GAT_HS} : Rows{Hg, GAT_H * GAT_C};
    const float s0 = att_s[hd * GAT_C + lane], s1 = att_s[hd * GAT_C + 64 + lane];
    const float d0 = att_d[hd * GAT_C + lane], d1 = att_d[hd * GAT_C + 64 + lane];
    for (int j = wave; j < N; j += GAT_THREADS / 64) {
        const float h0 = hr.p[(size_t)j * hr.stride + lane], h1 = hr.p[(size_t)j * hr.stride + 64 + lane];
        const float vs = wave_sum(h0 * s0 + h1 * s1), vd = wave_sum(h0 * d0 + h1 * d1);
        if (lane == 0) { l.as[j] = vs; l.ad[j] = vd; }
    }
    // edge list -> multiplicities (self loops dropped, out-of-range ids ignored, counts saturate at 255: reported through `status`)
    for (int e = tid; e < (complete ? 0 : E); e += GAT_THREADS) {
        const long long sj = edges[(size_t)(e0 + e) * 2 + 0], di = edges[(size_t)(e0 + e) * 2 + 1];
        if (sj != di && sj >= 0 && sj < N && di >= 0 && di < N) {
            const int idx = (int)di * npad + (int)sj;
            const unsigned sh = 8u * (idx & 3);
            const unsigned old = atomicAdd(&l.cnt[idx >> 2], 1u << sh);
            if (((old >> sh) & 255u) == 255u) {
                atomicSub(&l.cnt[idx >> 2], 1u << sh);
                if (status) atomicOr(status, 1);           // a (source, target) pair listed > 255 times: PyG would count them all
            }
        }
    }
    __syncthreads();
    unsigned char* cb = reinterpret_cast<unsigned char*>(l.cnt);
    for (int i = tid; i < N; i += GAT_THREADS) cb[i * npad + i] = 1;       // exactly one self loop per node
    __syncthreads();
    return hr;
}

// softmax row i for sources j = lane + 64 k: alpha a[k], pre-activations, max, denom
template <int NJ>
__device__ __forceinline__ void softmax_row(const GatLds& l, int i, int N, int npad, int lane, float (&a)[NJ],
                                            float (&pre)[NJ], float& m, float& den) {
    const unsigned char* cb = reinterpret_cast<const unsigned char*>(l.cnt);
    const float adi = l.ad[i];
    float c[NJ], e[NJ], p[NJ];
    float mloc = -INFINITY;
#pragma unroll
    for (int k = 0; k < NJ; ++k) {
        const int j = lane + 64 * k;
        c[k] = j < N ? (float)cb[i * npad + j] : 0.f;
        pre[k] = j < N ? l.as[j] + adi : 0.f;
        e[k] = lrelu(pre[k]);
        mloc = fmaxf(mloc, c[k] > 0.f ? e[k] : -INFINITY);
    }
    m = wave_max(mloc);
    float sloc = 0.f;
#pragma unroll
    for (int k = 0; k < NJ; ++k) {
        p[k] = c[k] > 0.f ? c[k] * __expf(e[k] - m) : 0.f;
        sloc += p[k];
    }
    den = wave_sum(sloc) + 1e-16f;
#pragma unroll
    for (int k = 0; k < NJ; ++k) a[k] = p[k] / den;
}

template <int NJ, bool LDSF>
__global__ __launch_bounds__(GAT_THREADS) void gat_attn_fwd_kernel(
    const float* __restrict__ H, const float* __restrict__ att_s, const float* __restrict__ att_d,
    const float* __restrict__ bias, const long long* __restrict__ edges, const int* __restrict__ node_off,
    const int* __restrict__ edge_off, float* __restrict__ out, int nmax, int* __restrict__ status,
    const unsigned char* __restrict__ complete) {
    extern __shared__ __attribute__((aligned(16))) float lds_raw[];
    const GatLds l = carve<NJ, LDSF>(lds_raw, nmax, false);
    const int g = blockIdx.x, hd = blockIdx.y;
    const int n0 = node_off[g], N = node_off[g + 1] - n0, e0 = edge_off[g], E = edge_off[g + 1] - e0;
    const int npad = (nmax + 3) & ~3;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (N <= 0) return;
    const Rows hr = gat_prologue<NJ, LDSF>(l, H, att_s, att_d, edges, n0, N, e0, E, hd, npad, status, complete && complete[g]);
    const float b0 = bias[hd * GAT_C + lane], b1 = bias[hd * GAT_C + 64 + lane];
    // GAT_TB targets per wave at a time: every h[j] row read feeds GAT_TB aggregates (the loop is LDS / L2 bound)
    for (int ib = wave * GAT_TB; ib < N; ib += (GAT_THREADS / 64) * GAT_TB) {
        float al[GAT_TB][NJ], acc0[GAT_TB], acc1[GAT_TB];
#pragma unroll
        for (int u = 0; u < GAT_TB; ++u) {
            float pre[NJ], m, den;
            acc0[u] = 0.f; acc1[u] = 0.f;
#pragma unroll
            for (int k = 0; k < NJ; ++k) al[u][k] = 0.f;
            if (ib + u < N) softmax_row<NJ>(l, ib + u, N, npad, lane, al[u], pre, m, den);
        }
#pragma unroll
        for (int k = 0; k < NJ; ++k)
            for (int jj = 0; jj < 64 && 64 * k + jj < N; ++jj) {
                const int j = 64 * k + jj;
                const float h0 = hr.p[(size_t)j * hr.stride + lane], h1 = hr.p[(size_t)j * hr.stride + 64 + lane];
#pragma unroll
                for (int u = 0; u < GAT_TB; ++u) {
                    const float a = __shfl(al[u][k], jj, 64);
                    acc0[u] = fmaf(a, h0, acc0[u]);
                    acc1[u] = fmaf(a, h1, acc1[u]);
                }
            }
#pragma unroll
        for (int u = 0; u < GAT_TB; ++u)
            if (ib + u < N) {
                float* o = out + (size_t)(n0 + ib + u) * (GAT_H * GAT_C) + hd * GAT_C;
                o[lane] = acc0[u] + b0;
                o[64 + lane] = acc1[u] + b1;
            }
    }
}

template <int NJ, bool LDSF>
__global__ __launch_bounds__(GAT_THREADS) void gat_attn_bwd_kernel(
    const float* __restrict__ H, const float* __restrict__ dO, const float* __restrict__ att_s,
    const float* __restrict__ att_d, const long long* __restrict__ edges, const int* __restrict__ node_off,
    const int* __restrict__ edge_off, float* __restrict__ dH, float* __restrict__ d_att_s,
    float* __restrict__ d_att_d, int nmax, const unsigned char* __restrict__ complete) {
    constexpr int MAXN = NJ * 64;
    extern __shared__ __attribute__((aligned(16))) float lds_raw[];
    const GatLds l = carve<NJ, LDSF>(lds_raw, nmax, true);
    const int g = blockIdx.x, hd = blockIdx.y;
    const int n0 = node_off[g], N = node_off[g + 1] - n0, e0 = edge_off[g], E = edge_off[g + 1] - e0;
    const int npad = (nmax + 3) & ~3;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (N <= 0) return;
    const float* Dg = dO + (size_t)n0 * (GAT_H * GAT_C) + hd * GAT_C;
    if (LDSF)
        for (int e = tid; e < N * GAT_C; e += GAT_THREADS) {
            const int j = e >> 7, c = e & 127;
            l.dos[j * GAT_HS + c] = Dg[(size_t)j * (GAT_H * GAT_C) + c];
        }
    for (int j = tid; j < MAXN; j += GAT_THREADS) l.das[j] = 0.f;
    const Rows hr = gat_prologue<NJ, LDSF>(l, H, att_s, att_d, edges, n0, N, e0, E, hd, npad, nullptr, complete && complete[g]);
    const Rows dr = LDSF ? Rows{l.dos, GAT_HS} : Rows{Dg, GAT_H * GAT_C};

    // ---- phase 1: per target row i -> d a_d[i], partial d a_s[j], row max / denom
    float das[NJ];
    int js[NJ];
#pragma unroll
    for (int k = 0; k < NJ; ++k) { das[k] = 0.f; js[k] = lane + 64 * k < N ? lane + 64 * k : 0; }
    for (int ib = wave * GAT_TB; ib < N; ib += (GAT_THREADS / 64) * GAT_TB) {
        float al[GAT_TB][NJ], pre[GAT_TB][NJ], m[GAT_TB], den[GAT_TB], da[GAT_TB][NJ];
#pragma unroll
        for (int u = 0; u < GAT_TB; ++u) {
            m[u] = 0.f; den[u] = 1.f;
#pragma unroll
            for (int k = 0; k < NJ; ++k) { al[u][k] = 0.f; pre[u][k] = 0.f; da[u][k] = 0.f; }
            if (ib + u < N) softmax_row<NJ>(l, ib + u, N, npad, lane, al[u], pre[u], m[u], den[u]);
        }
        // d alpha_ij = <dO[i], h[j]> for GAT_TB targets i at once: the h reads per channel are shared
        for (int c = 0; c < GAT_C; ++c) {
            float hv[NJ];
#pragma unroll
            for (int k = 0; k < NJ; ++k) hv[k] = hr.p[(size_t)js[k] * hr.stride + c];
#pragma unroll
            for (int u = 0; u < GAT_TB; ++u) {
                const float d = dr.p[(size_t)min(ib + u, N - 1) * dr.stride + c];
#pragma unroll
                for (int k = 0; k < NJ; ++k) da[u][k] = fmaf(d, hv[k], da[u][k]);
            }
        }
#pragma unroll
        for (int u = 0; u < GAT_TB; ++u) {
            if (ib + u >= N) continue;
            float dot = 0.f;
#pragma unroll
            for (int k = 0; k < NJ; ++k) dot = fmaf(al[u][k], da[u][k], dot);
            const float s = wave_sum(dot);
            float dsum = 0.f;
#pragma unroll
            for (int k = 0; k < NJ; ++k) {
                const float ds = al[u][k] * (da[u][k] - s) * (pre[u][k] > 0.f ? 1.f : GAT_SLOPE);
                das[k] += ds;
                dsum += ds;
            }
            const float dd = wave_sum(dsum);
            if (lane == 0) { l.dad[ib + u] = dd; l.mx[ib + u] = m[u]; l.den[ib + u] = den[u]; }
        }
    }
#pragma unroll
    for (int k = 0; k < NJ; ++k)
        if (lane + 64 * k < N) atomicAdd(&l.das[lane + 64 * k], das[k]);
    __syncthreads();

    // ---- phase 2: per source j -> dH[j] = sum_i alpha_ij dO[i] + d a_s[j] att_s + d a_d[j] att_d ; d att
    const unsigned char* cb = reinterpret_cast<const unsigned char*>(l.cnt);
    const float s0 = att_s[hd * GAT_C + lane], s1 = att_s[hd * GAT_C + 64 + lane];
    const float d0 = att_d[hd * GAT_C + lane], d1 = att_d[hd * GAT_C + 64 + lane];
    float gs0 = 0.f, gs1 = 0.f, gd0 = 0.f, gd1 = 0.f;
    for (int jb = wave * GAT_TB; jb < N; jb += (GAT_THREADS / 64) * GAT_TB) {
        // alpha_ij for targets i = lane + 64 k (vectorised over targets) of GAT_TB sources j, then broadcast per i
        float al[GAT_TB][NJ], acc0[GAT_TB], acc1[GAT_TB];
#pragma unroll
        for (int u = 0; u < GAT_TB; ++u) {
            acc0[u] = 0.f; acc1[u] = 0.f;
            const int j = jb + u;
            const float asj = j < N ? l.as[j] : 0.f;
#pragma unroll
            for (int k = 0; k < NJ; ++k) {
                al[u][k] = 0.f;
                const int i = lane + 64 * k;
                if (j < N && i < N) {
                    const float c = (float)cb[i * npad + j];
                    if (c > 0.f) al[u][k] = c * __expf(lrelu(asj + l.ad[i]) - l.mx[i]) / l.den[i];
                }
            }
        }
#pragma unroll
        for (int k = 0; k < NJ; ++k)
            for (int ii = 0; ii < 64 && 64 * k + ii < N; ++ii) {
                const int i = 64 * k + ii;
                const float g0 = dr.p[(size_t)i * dr.stride + lane], g1 = dr.p[(size_t)i * dr.stride + 64 + lane];
#pragma unroll
                for (int u = 0; u < GAT_TB; ++u) {
                    const float a = __shfl(al[u][k], ii, 64);
                    acc0[u] = fmaf(a, g0, acc0[u]);
                    acc1[u] = fmaf(a, g1, acc1[u]);
                }
            }
#pragma unroll
        for (int u = 0; u < GAT_TB; ++u) {
            const int j = jb + u;
            if (j >= N) continue;
            const float dasj = l.das[j], dadj = l.dad[j];
            float* o = dH + (size_t)(n0 + j) * (GAT_H * GAT_C) + hd * GAT_C;
            o[lane] = acc0[u] + dasj * s0 + dadj * d0;
            o[64 + lane] = acc1[u] + dasj * s1 + dadj * d1;
            const float h0 = hr.p[(size_t)j * hr.stride + lane], h1 = hr.p[(size_t)j * hr.stride + 64 + lane];
            gs0 = fmaf(dasj, h0, gs0); gs1 = fmaf(dasj, h1, gs1);
            gd0 = fmaf(dadj, h0, gd0); gd1 = fmaf(dadj, h1, gd1);
        }
    }
    atomicAdd(d_att_s + hd * GAT_C + lane, gs0);
    atomicAdd(d_att_s + hd * GAT_C + 64 + lane, gs1);
    atomicAdd(d_att_d + hd * GAT_C + lane, gd0);
    atomicAdd(d_att_d + hd * GAT_C + 64 + lane, gd1);
}

// ELU between the layers (gat.py:45-46) and its derivative
__global__ void elu_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, size_t n) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const float v = x[i];
        y[i] = v > 0.f ? v : expm1f(v);
    }
}
__global__ void elu_bwd_kernel(const float* __restrict__ x, const float* __restrict__ gy, float* __restrict__ gx, size_t n) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const float v = x[i];
        // exp in fp64, rounded once.  Not expf: under -ffp-contract=fast the compiler's float expansion of it, 2^((p - rint(p)) + p_lo) with
        // p = fl(v log2e), has p - rint(p) fused into fma(v, log2e, -rint(p)) and then adds the product's rounding error p_lo a second time --
        // up to 40 ulp for v in [-90, -2.5] (tests/test_elementwise_gpu.py holds this kernel to 4 ulp).
        gx[i] = v > 0.f ? gy[i] : gy[i] * (float)exp((double)v);
    }
}

int check_common(int G, int nmax, const char* who) {
    if (G < 0 || nmax < 0) { sga_set_error("%s: negative size", who); return SGA_ERR_ARG; }
    if (nmax > GAT_MAXN_BIG) {
        sga_set_error("%s: a graph has %d nodes; the GAT kernels support at most %d per graph", who, nmax, GAT_MAXN_BIG);
        return SGA_ERR_ARG;
    }
    return SGA_OK;
}

// the launches of the 2 x 128 kernels: features LDS-resident exactly up to GAT_MAXN nodes
void launch_fwd_2x128(int G, hipStream_t s, const float* H, const float* att_s, const float* att_d, const float* bias, const long long* edges,
                      const int* node_off, const int* edge_off, float* out, int nmax, int* status, const unsigned char* complete) {
    const bool small = nmax <= GAT_MAXN;
    const size_t lds = gat_lds_bytes(nmax, false, small ? 2 : 4, small);
    auto k = small ? gat_attn_fwd_kernel<2, true> : gat_attn_fwd_kernel<4, false>;      // 129..256 nodes: features from global memory
    hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(k, dim3(G, GAT_H), dim3(GAT_THREADS), lds, s, H, att_s, att_d, bias, edges, node_off, edge_off, out, nmax, status, complete);
}

void launch_bwd_2x128(int G, hipStream_t s, const float* H, const float* dO, const float* att_s, const float* att_d, const long long* edges,
                      const int* node_off, const int* edge_off, float* dH, float* d_att_s, float* d_att_d, int nmax, const unsigned char* complete) {
    const bool small = nmax <= GAT_MAXN;
    const size_t lds = gat_lds_bytes(nmax, true, small ? 2 : 4, small);
    auto k = small ? gat_attn_bwd_kernel<2, true> : gat_attn_bwd_kernel<4, false>;
    hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(k, dim3(G, GAT_H), dim3(GAT_THREADS), lds, s, H, dO, att_s, att_d, edges, node_off, edge_off, dH, d_att_s, d_att_d, nmax, complete);
}

}  // namespace

// flags[g] = 1 iff graph g lists every ordered pair i != j exactly once and nothing else (E = N (N - 1), every edge in range, no self
// loop, no duplicate -- an N x N bitmap in LDS catches duplicates whatever the ORDER of the list: preprocess.py writes the annotated
// relations first and the supplemented 'none' pairs after them).
__global__ __launch_bounds__(GAT_THREADS) void gat_complete_kernel(const long long* __restrict__ edges, const int* __restrict__ node_off,
                                                                   const int* __restrict__ edge_off, unsigned char* __restrict__ flags) {
    __shared__ unsigned bits[GAT_MAXN_BIG * GAT_MAXN_BIG / 32];
    const int g = blockIdx.x, tid = threadIdx.x;
    const int N = node_off[g + 1] - node_off[g], e0 = edge_off[g], E = edge_off[g + 1] - e0;
    if (N <= 0 || N > GAT_MAXN_BIG || (long long)E != (long long)N * (N - 1)) { if (tid == 0) flags[g] = 0; return; }   // uniform
    for (int w = tid; w < (N * N + 31) / 32; w += GAT_THREADS) bits[w] = 0u;
    __syncthreads();
    int bad = 0;
    for (int e = tid; e < E; e += GAT_THREADS) {
        const long long sj = edges[(size_t)(e0 + e) * 2 + 0], di = edges[(size_t)(e0 + e) * 2 + 1];
        if (sj == di || sj < 0 || sj >= N || di < 0 || di >= N) { bad = 1; continue; }
        const int idx = (int)di * N + (int)sj;
        if (atomicOr(&bits[idx >> 5], 1u << (idx & 31)) & (1u << (idx & 31))) bad = 1;
    }
    bad = __syncthreads_or(bad);
    if (tid == 0) flags[g] = bad ? 0 : 1;
}

extern "C" int sga_gat_complete_flags(const int64_t* edges, const int32_t* node_off, const int32_t* edge_off, int G, uint8_t* flags, void* stream) {
    if (G == 0) return SGA_OK;
    SGA_CHECK_ARG(node_off && edge_off && flags && G > 0, "sga_gat_complete_flags: bad argument");
    hipLaunchKernelGGL(gat_complete_kernel, dim3(G), dim3(GAT_THREADS), 0, static_cast<hipStream_t>(stream),
                       reinterpret_cast<const long long*>(edges), node_off, edge_off, flags);
    SGA_CHECK_LAUNCH("sga_gat_complete_flags");
    return SGA_OK;
}

extern "C" int sga_elu_fwd(const float* x, float* y, size_t n, void* stream) {
    if (n == 0) return SGA_OK;
    SGA_CHECK_ARG(x && y, "sga_elu_fwd: null pointer");
    size_t g = (n + 255) / 256; if (g > 8192) g = 8192;
    hipLaunchKernelGGL(elu_fwd_kernel, dim3((unsigned)g), dim3(256), 0, static_cast<hipStream_t>(stream), x, y, n);
    SGA_CHECK_LAUNCH("sga_elu_fwd");
    return SGA_OK;
}

extern "C" int sga_elu_bwd(const float* x, const float* gy, float* gx, size_t n, void* stream) {
    if (n == 0) return SGA_OK;
    SGA_CHECK_ARG(x && gy && gx, "sga_elu_bwd: null pointer");
    size_t g = (n + 255) / 256; if (g > 8192) g = 8192;
    hipLaunchKernelGGL(elu_bwd_kernel, dim3((unsigned)g), dim3(256), 0, static_cast<hipStream_t>(stream), x, gy, gx, n);
    SGA_CHECK_LAUNCH("sga_elu_bwd");
    return SGA_OK;
}

// ---- the general form: GATConv(in, C, heads) for any heads >= 1 and 1 <= C <= 256 (every stack reference gat.py:34-37 can build) ----
// Same algorithm, arithmetic and order as the kernels above, which the entry points launch at 2 x 128.  heads and C are run-time values
// (grid y, row stride heads * C); lanes span the channels in CJ = ceil(C / 64) slots (channel c = lane + 64 k), a template parameter.  Only
// the LAST slot can be ragged: its lanes past C read channel C - 1 again (a valid address, no branch in the inner loops), enter every dot
// product with weight 0 and are never written.  The LDS row stride is C | 1: odd for every C, so lanes walking down a column (backward
// phase 1: one source row per lane) and lanes walking along a row both hit 64 different banks.  NJ (source slots per lane) follows the
// node count as above; whether the head's feature rows live in LDS (LDSF) is decided on the host, per launch, from C, nmax and the
// 160 KiB of LDS a CU has -- so NJ = 4 with resident features exists here (narrow heads), and NJ = 2 without (wide heads, backward).
namespace {

constexpr int GAT_CMAX = 256;                      // channels per head (CJ <= 4)
constexpr size_t GAT_LDS_BUDGET = 160 * 1024;      // LDS of one CU (gfx950): one workgroup may have all of it

inline int gat_hs(int C) { return C | 1; }
inline int gat_nj(int nmax) { return nmax <= GAT_MAXN ? 2 : 4; }

inline size_t gat_lds_bytes_hc(int nmax, bool bwd, int C, bool ldsf) {
    const int npad = (nmax + 3) & ~3;
    return sizeof(float) * ((ldsf ? (size_t)nmax * gat_hs(C) * (bwd ? 2 : 1) : 0) + 6 * (size_t)gat_nj(nmax) * 64) + (size_t)nmax * npad;
}

inline bool gat_fits_lds(int nmax, bool bwd, int C) { return gat_lds_bytes_hc(nmax, bwd, C, true) <= GAT_LDS_BUDGET; }

template <int NJ, bool LDSF>
__device__ __forceinline__ GatLds carve_hc(float* base, int nmax, int hs, bool bwd) {
    constexpr int MAXN = NJ * 64;
    GatLds l;
    float* p = base;
    l.hs = p; if (LDSF) p += nmax * hs;
    l.dos = p; if (LDSF && bwd) p += nmax * hs;
    l.as = p; p += MAXN;
    l.ad = p; p += MAXN;
    l.mx = p; p += MAXN;
    l.den = p; p += MAXN;
    l.das = p; p += MAXN;
    l.dad = p; p += MAXN;
    l.cnt = reinterpret_cast<unsigned*>(p);
    return l;
}

// N rows of C channels, global (row stride ld) -> LDS (row stride hs): one wave per row, lanes along the row
template <int CJ>
__device__ __forceinline__ void rows_to_lds(float* dst, int hs, const float* __restrict__ src, int ld, int N, int C) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int j = wave; j < N; j += GAT_THREADS / 64)
#pragma unroll
        for (int k = 0; k < CJ; ++k) {
            const int c = lane + 64 * k;
            if (c < C) dst[j * hs + c] = src[(size_t)j * ld + c];
        }
}

// common prologue (gat_prologue for run-time heads / C): features (LDSF), the logits' node parts, the multiplicity matrix
template <int NJ, int CJ, bool LDSF>
__device__ __forceinline__ Rows gat_prologue_hc(const GatLds& l, const float* __restrict__ H, const float* __restrict__ att_s,
                                                const float* __restrict__ att_d, const long long* __restrict__ edges,
                                                int n0, int N, int e0, int E, int hd, int heads, int C, int hs, int npad,
                                                int* status, bool complete) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int HC = heads * C;
    const float* Hg = H + (size_t)n0 * HC + hd * C;
    if (LDSF) rows_to_lds<CJ>(l.hs, hs, Hg, HC, N, C);
    if (complete) {                                        // every multiplicity is 1: the edge list is never touched
        for (int e = tid; e < N * (npad >> 2); e += GAT_THREADS) {
            const int j4 = (e % (npad >> 2)) * 4;
            l.cnt[e] = (j4 + 0 < N ? 1u : 0u) | (j4 + 1 < N ? 0x100u : 0u) | (j4 + 2 < N ? 0x10000u : 0u) | (j4 + 3 < N ? 0x1000000u : 0u);
        }
    } else {
        for (int e = tid; e < N * (npad >> 2); e += GAT_THREADS) l.cnt[e] = 0u;
    }
    __syncthreads();
    const Rows hr = LDSF ? Rows{l.hs, hs} : Rows{Hg, HC};
    float sv[CJ], dv[CJ];
    int cc[CJ];
#pragma unroll
    for (int k = 0; k < CJ; ++k) {
        const int c = lane + 64 * k;
        cc[k] = min(c, C - 1);
        sv[k] = c < C ? att_s[hd * C + c] : 0.f;
        dv[k] = c < C ? att_d[hd * C + c] : 0.f;
    }
    for (int j = wave; j < N; j += GAT_THREADS / 64) {
        float ps = 0.f, pd = 0.f;
#pragma unroll
        for (int k = 0; k < CJ; ++k) {
            const float h = hr.p[(size_t)j * hr.stride + cc[k]];
            ps = fmaf(h, sv[k], ps);
            pd = fmaf(h, dv[k], pd);
        }
        const float vs = wave_sum(ps), vd = wave_sum(pd);
        if (lane == 0) { l.as[j] = vs; l.ad[j] = vd; }
    }
    // edge list -> multiplicities (self loops dropped, out-of-range ids ignored, counts saturate at 255: reported through `status`)
    for (int e = tid; e < (complete ? 0 : E); e += GAT_THREADS) {
        const long long sj = edges[(size_t)(e0 + e) * 2 + 0], di = edges[(size_t)(e0 + e) * 2 + 1];
        if (sj != di && sj >= 0 && sj < N && di >= 0 && di < N) {
            const int idx = (int)di * npad + (int)sj;
            const unsigned sh = 8u * (idx & 3);
            const unsigned old = atomicAdd(&l.cnt[idx >> 2], 1u << sh);
            if (((old >> sh) & 255u) == 255u) {
                atomicSub(&l.cnt[idx >> 2], 1u << sh);
                if (status) atomicOr(status, 1);
            }
        }
    }
    __syncthreads();
    unsigned char* cb = reinterpret_cast<unsigned char*>(l.cnt);
    for (int i = tid; i < N; i += GAT_THREADS) cb[i * npad + i] = 1;       // exactly one self loop per node
    __syncthreads();
    return hr;
}

template <int NJ, int CJ, bool LDSF>
__global__ __launch_bounds__(GAT_THREADS) void gat_attn_fwd_hc_kernel(
    const float* __restrict__ H, const float* __restrict__ att_s, const float* __restrict__ att_d,
    const float* __restrict__ bias, const long long* __restrict__ edges, const int* __restrict__ node_off,
    const int* __restrict__ edge_off, float* __restrict__ out, int nmax, int C, int* __restrict__ status,
    const unsigned char* __restrict__ complete) {
    extern __shared__ __attribute__((aligned(16))) float lds_raw[];
    const int hs = C | 1, heads = gridDim.y, HC = heads * C;
    const GatLds l = carve_hc<NJ, LDSF>(lds_raw, nmax, hs, false);
    const int g = blockIdx.x, hd = blockIdx.y;
    const int n0 = node_off[g], N = node_off[g + 1] - n0, e0 = edge_off[g], E = edge_off[g + 1] - e0;
    const int npad = (nmax + 3) & ~3;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (N <= 0) return;
    const Rows hr = gat_prologue_hc<NJ, CJ, LDSF>(l, H, att_s, att_d, edges, n0, N, e0, E, hd, heads, C, hs, npad, status, complete && complete[g]);
    int cc[CJ];
    float bv[CJ];
#pragma unroll
    for (int k = 0; k < CJ; ++k) { cc[k] = min(lane + 64 * k, C - 1); bv[k] = bias[hd * C + cc[k]]; }
    for (int ib = wave * GAT_TB; ib < N; ib += (GAT_THREADS / 64) * GAT_TB) {
        float al[GAT_TB][NJ], acc[GAT_TB][CJ];
#pragma unroll
        for (int u = 0; u < GAT_TB; ++u) {
            float pre[NJ], m, den;
#pragma unroll
            for (int q = 0; q < CJ; ++q) acc[u][q] = 0.f;
#pragma unroll
            for (int k = 0; k < NJ; ++k) al[u][k] = 0.f;
            if (ib + u < N) softmax_row<NJ>(l, ib + u, N, npad, lane, al[u], pre, m, den);
        }
#pragma unroll
        for (int k = 0; k < NJ; ++k)
            for (int jj = 0; jj < 64 && 64 * k + jj < N; ++jj) {
                const int j = 64 * k + jj;
                float h[CJ];
#pragma unroll
                for (int q = 0; q < CJ; ++q) h[q] = hr.p[(size_t)j * hr.stride + cc[q]];
#pragma unroll
                for (int u = 0; u < GAT_TB; ++u) {
                    const float a = __shfl(al[u][k], jj, 64);
#pragma unroll
                    for (int q = 0; q < CJ; ++q) acc[u][q] = fmaf(a, h[q], acc[u][q]);
                }
            }
#pragma unroll
        for (int u = 0; u < GAT_TB; ++u)
            if (ib + u < N) {
                float* o = out + (size_t)(n0 + ib + u) * HC + hd * C;
#pragma unroll
                for (int q = 0; q < CJ; ++q)
                    if (lane + 64 * q < C) o[lane + 64 * q] = acc[u][q] + bv[q];
            }
    }
}

template <int NJ, int CJ, bool LDSF>
__global__ __launch_bounds__(GAT_THREADS) void gat_attn_bwd_hc_kernel(
    const float* __restrict__ H, const float* __restrict__ dO, const float* __restrict__ att_s,
    const float* __restrict__ att_d, const long long* __restrict__ edges, const int* __restrict__ node_off,
    const int* __restrict__ edge_off, float* __restrict__ dH, float* __restrict__ d_att_s,
    float* __restrict__ d_att_d, int nmax, int C, const unsigned char* __restrict__ complete) {
    constexpr int MAXN = NJ * 64;
    extern __shared__ __attribute__((aligned(16))) float lds_raw[];
    const int hs = C | 1, heads = gridDim.y, HC = heads * C;
    const GatLds l = carve_hc<NJ, LDSF>(lds_raw, nmax, hs, true);
    const int g = blockIdx.x, hd = blockIdx.y;
    const int n0 = node_off[g], N = node_off[g + 1] - n0, e0 = edge_off[g], E = edge_off[g + 1] - e0;
    const int npad = (nmax + 3) & ~3;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (N <= 0) return;
    const float* Dg = dO + (size_t)n0 * HC + hd * C;
    if (LDSF) rows_to_lds<CJ>(l.dos, hs, Dg, HC, N, C);
    for (int j = tid; j < MAXN; j += GAT_THREADS) l.das[j] = 0.f;
    const Rows hr = gat_prologue_hc<NJ, CJ, LDSF>(l, H, att_s, att_d, edges, n0, N, e0, E, hd, heads, C, hs, npad, nullptr, complete && complete[g]);
    const Rows dr = LDSF ? Rows{l.dos, hs} : Rows{Dg, HC};

    // ---- phase 1: per target row i -> d a_d[i], partial d a_s[j], row max / denom
    float das[NJ];
    int js[NJ];
#pragma unroll
    for (int k = 0; k < NJ; ++k) { das[k] = 0.f; js[k] = lane + 64 * k < N ? lane + 64 * k : 0; }
    for (int ib = wave * GAT_TB; ib < N; ib += (GAT_THREADS / 64) * GAT_TB) {
        float al[GAT_TB][NJ], pre[GAT_TB][NJ], m[GAT_TB], den[GAT_TB], da[GAT_TB][NJ];
#pragma unroll
        for (int u = 0; u < GAT_TB; ++u) {
            m[u] = 0.f; den[u] = 1.f;
#pragma unroll
            for (int k = 0; k < NJ; ++k) { al[u][k] = 0.f; pre[u][k] = 0.f; da[u][k] = 0.f; }
            if (ib + u < N) softmax_row<NJ>(l, ib + u, N, npad, lane, al[u], pre[u], m[u], den[u]);
        }
        // d alpha_ij = <dO[i], h[j]> for GAT_TB targets i at once: the h reads per channel are shared
        for (int c = 0; c < C; ++c) {
            float hv[NJ];
#pragma unroll
            for (int k = 0; k < NJ; ++k) hv[k] = hr.p[(size_t)js[k] * hr.stride + c];
#pragma unroll
            for (int u = 0; u < GAT_TB; ++u) {
                const float d = dr.p[(size_t)min(ib + u, N - 1) * dr.stride + c];
#pragma unroll
                for (int k = 0; k < NJ; ++k) da[u][k] = fmaf(d, hv[k], da[u][k]);
            }
        }
#pragma unroll
        for (int u = 0; u < GAT_TB; ++u) {
            if (ib + u >= N) continue;
            float dot = 0.f;
#pragma unroll
            for (int k = 0; k < NJ; ++k) dot = fmaf(al[u][k], da[u][k], dot);
            const float s = wave_sum(dot);
            float dsum = 0.f;
#pragma unroll
            for (int k = 0; k < NJ; ++k) {
                const float ds = al[u][k] * (da[u][k] - s) * (pre[u][k] > 0.f ? 1.f : GAT_SLOPE);
                das[k] += ds;
                dsum += ds;
            }
            const float dd = wave_sum(dsum);
            if (lane == 0) { l.dad[ib + u] = dd; l.mx[ib + u] = m[u]; l.den[ib + u] = den[u]; }
        }
    }
#pragma unroll
    for (int k = 0; k < NJ; ++k)
        if (lane + 64 * k < N) atomicAdd(&l.das[lane + 64 * k], das[k]);
    __syncthreads();

    // ---- phase 2: per source j -> dH[j] = sum_i alpha_ij dO[i] + d a_s[j] att_s + d a_d[j] att_d ; d att
    const unsigned char* cb = reinterpret_cast<const unsigned char*>(l.cnt);
    int cc[CJ];
    float sv[CJ], dv[CJ], gs[CJ], gd[CJ];
#pragma unroll
    for (int q = 0; q < CJ; ++q) {
        cc[q] = min(lane + 64 * q, C - 1);
        sv[q] = att_s[hd * C + cc[q]];
        dv[q] = att_d[hd * C + cc[q]];
        gs[q] = 0.f; gd[q] = 0.f;
    }
    for (int jb = wave * GAT_TB; jb < N; jb += (GAT_THREADS / 64) * GAT_TB) {
        float al[GAT_TB][NJ], acc[GAT_TB][CJ];
#pragma unroll
        for (int u = 0; u < GAT_TB; ++u) {
#pragma unroll
            for (int q = 0; q < CJ; ++q) acc[u][q] = 0.f;
            const int j = jb + u;
            const float asj = j < N ? l.as[j] : 0.f;
#pragma unroll
            for (int k = 0; k < NJ; ++k) {
                al[u][k] = 0.f;
                const int i = lane + 64 * k;
                if (j < N && i < N) {
                    const float c = (float)cb[i * npad + j];
                    if (c > 0.f) al[u][k] = c * __expf(lrelu(asj + l.ad[i]) - l.mx[i]) / l.den[i];
                }
            }
        }
#pragma unroll
        for (int k = 0; k < NJ; ++k)
            for (int ii = 0; ii < 64 && 64 * k + ii < N; ++ii) {
                const int i = 64 * k + ii;
                float gv[CJ];
#pragma unroll
                for (int q = 0; q < CJ; ++q) gv[q] = dr.p[(size_t)i * dr.stride + cc[q]];
#pragma unroll
                for (int u = 0; u < GAT_TB; ++u) {
                    const float a = __shfl(al[u][k], ii, 64);
#pragma unroll
                    for (int q = 0; q < CJ; ++q) acc[u][q] = fmaf(a, gv[q], acc[u][q]);
                }
            }
#pragma unroll
        for (int u = 0; u < GAT_TB; ++u) {
            const int j = jb + u;
            if (j >= N) continue;
            const float dasj = l.das[j], dadj = l.dad[j];
            float* o = dH + (size_t)(n0 + j) * HC + hd * C;
#pragma unroll
            for (int q = 0; q < CJ; ++q) {
                if (lane + 64 * q < C) o[lane + 64 * q] = acc[u][q] + dasj * sv[q] + dadj * dv[q];
                const float h = hr.p[(size_t)j * hr.stride + cc[q]];
                gs[q] = fmaf(dasj, h, gs[q]);
                gd[q] = fmaf(dadj, h, gd[q]);
            }
        }
    }
#pragma unroll
    for (int q = 0; q < CJ; ++q)
        if (lane + 64 * q < C) {
            atomicAdd(d_att_s + hd * C + lane + 64 * q, gs[q]);
            atomicAdd(d_att_d + hd * C + lane + 64 * q, gd[q]);
        }
}

int check_hc(int heads, int channels, const char* who) {
    if (heads < 1) { sga_set_error("%s: heads %d < 1", who, heads); return SGA_ERR_ARG; }
    if (channels < 1 || channels > GAT_CMAX) {
        sga_set_error("%s: channels %d outside 1 .. %d per head", who, channels, GAT_CMAX);
        return SGA_ERR_ARG;
    }
    return SGA_OK;
}

template <int NJ, int CJ, bool LDSF>
void launch_fwd_hc(size_t lds, int G, int heads, hipStream_t s, const float* H, const float* att_s, const float* att_d, const float* bias,
                   const long long* edges, const int* node_off, const int* edge_off, float* out, int nmax, int C, int* status,
                   const unsigned char* complete) {
    auto k = gat_attn_fwd_hc_kernel<NJ, CJ, LDSF>;
    hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(k, dim3(G, heads), dim3(GAT_THREADS), lds, s, H, att_s, att_d, bias, edges, node_off, edge_off, out, nmax, C, status, complete);
}

template <int NJ, int CJ, bool LDSF>
void launch_bwd_hc(size_t lds, int G, int heads, hipStream_t s, const float* H, const float* dO, const float* att_s, const float* att_d,
                   const long long* edges, const int* node_off, const int* edge_off, float* dH, float* d_att_s, float* d_att_d, int nmax,
                   int C, const unsigned char* complete) {
    auto k = gat_attn_bwd_hc_kernel<NJ, CJ, LDSF>;
    hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(k, dim3(G, heads), dim3(GAT_THREADS), lds, s, H, dO, att_s, att_d, edges, node_off, edge_off, dH, d_att_s, d_att_d, nmax, C, complete);
}

// FN<NJ, CJ, LDSF>(...) for the run-time (nj in {2, 4}, cj in 1 .. 4, ldsf)
#define GAT_HC_CJ(FN, NJ, LDSF, ...)                         \
    switch (cj) {                                            \
        case 1: FN<NJ, 1, LDSF>(__VA_ARGS__); break;         \
        case 2: FN<NJ, 2, LDSF>(__VA_ARGS__); break;         \
        case 3: FN<NJ, 3, LDSF>(__VA_ARGS__); break;         \
        default: FN<NJ, 4, LDSF>(__VA_ARGS__); break;        \
    }
#define GAT_HC_DISPATCH(FN, ...)                                                \
    do {                                                                        \
        if (nj == 2 && ldsf) { GAT_HC_CJ(FN, 2, true, __VA_ARGS__) }            \
        else if (nj == 2) { GAT_HC_CJ(FN, 2, false, __VA_ARGS__) }              \
        else if (ldsf) { GAT_HC_CJ(FN, 4, true, __VA_ARGS__) }                  \
        else { GAT_HC_CJ(FN, 4, false, __VA_ARGS__) }                           \
    } while (0)

}  // namespace

// the GENERAL kernels' boundary: the 2 x 128 launch (launch_fwd_2x128 / launch_bwd_2x128) has its own, GAT_MAXN nodes in both directions
extern "C" int sga_gat_lds_nodes(int channels, int bwd) {
    if (channels < 1 || channels > GAT_CMAX) {
        sga_set_error("sga_gat_lds_nodes: channels %d outside 1 .. %d per head", channels, GAT_CMAX);
        return -1;
    }
    int n = 0;
    while (n < GAT_MAXN_BIG && gat_fits_lds(n + 1, bwd != 0, channels)) ++n;      // the byte count grows with the node count
    return n;
}

extern "C" int sga_gat_attn_fwd_hc(const float* H, int heads, int channels, const float* att_src, const float* att_dst, const float* bias,
                                   const int64_t* edges, const int32_t* node_off, const int32_t* edge_off, int G, int nmax,
                                   float* out, int32_t* status, const uint8_t* complete, void* stream) {
    int rc = check_hc(heads, channels, "sga_gat_attn_fwd_hc");
    if (rc) return rc;
    rc = check_common(G, nmax, "sga_gat_attn_fwd_hc");
    if (rc) return rc;
    if (G == 0 || nmax == 0) return SGA_OK;
    SGA_CHECK_ARG(H && att_src && att_dst && bias && node_off && edge_off && out, "sga_gat_attn_fwd_hc: null pointer");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const long long* e = reinterpret_cast<const long long*>(edges);
    if (heads == GAT_H && channels == GAT_C) {
        launch_fwd_2x128(G, s, H, att_src, att_dst, bias, e, node_off, edge_off, out, nmax, status, complete);
    } else {
        const int nj = gat_nj(nmax), cj = (channels + 63) / 64;
        const bool ldsf = gat_fits_lds(nmax, false, channels);
        const size_t lds = gat_lds_bytes_hc(nmax, false, channels, ldsf);
        GAT_HC_DISPATCH(launch_fwd_hc, lds, G, heads, s, H, att_src, att_dst, bias, e, node_off, edge_off, out, nmax, channels, status, complete);
    }
    SGA_CHECK_LAUNCH("sga_gat_attn_fwd_hc");
    return SGA_OK;
}

extern "C" int sga_gat_attn_bwd_hc(const float* H, const float* dO, int heads, int channels, const float* att_src, const float* att_dst,
                                   const int64_t* edges, const int32_t* node_off, const int32_t* edge_off, int G, int nmax, float* dH,
                                   float* d_att_src, float* d_att_dst, const uint8_t* complete, void* stream) {
    int rc = check_hc(heads, channels, "sga_gat_attn_bwd_hc");
    if (rc) return rc;
    rc = check_common(G, nmax, "sga_gat_attn_bwd_hc");
    if (rc) return rc;
    SGA_CHECK_ARG(((G == 0 || nmax == 0) || (H && dO && node_off && edge_off && dH)) && att_src && att_dst && d_att_src && d_att_dst, "sga_gat_attn_bwd_hc: null pointer");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t hc = (size_t)heads * channels;
    if (d_att_dst == d_att_src + hc) {                                // one flat buffer: one launch
        hipMemsetAsync(d_att_src, 0, 2 * hc * sizeof(float), s);
    } else {
        hipMemsetAsync(d_att_src, 0, hc * sizeof(float), s);
        hipMemsetAsync(d_att_dst, 0, hc * sizeof(float), s);
    }
    if (G == 0 || nmax == 0) return SGA_OK;
    const long long* e = reinterpret_cast<const long long*>(edges);
    if (heads == GAT_H && channels == GAT_C) {
        launch_bwd_2x128(G, s, H, dO, att_src, att_dst, e, node_off, edge_off, dH, d_att_src, d_att_dst, nmax, complete);
    } else {
        const int nj = gat_nj(nmax), cj = (channels + 63) / 64;
        const bool ldsf = gat_fits_lds(nmax, true, channels);
        const size_t lds = gat_lds_bytes_hc(nmax, true, channels, ldsf);
        GAT_HC_DISPATCH(launch_bwd_hc, lds, G, heads, s, H, dO, att_src, att_dst, e, node_off, edge_off, dH, d_att_src, d_att_dst, nmax, channels, complete);
    }
    SGA_CHECK_LAUNCH("sga_gat_attn_bwd_hc");
    return SGA_OK;
}
