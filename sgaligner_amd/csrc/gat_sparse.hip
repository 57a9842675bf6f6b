// GAT attention over a compressed edge list (CSR): the route for graphs of ANY size, fwd + bwd, without atomics.
//
// gat.hip keeps a dense N x N multiplicity matrix of one graph in LDS, which caps a graph at 256 nodes and a (source, target) pair at 255
// copies.  Here the edge lists of a batch are turned ONCE into a canonical structure over batch-global node ids (rules of gat_prologue:
// input self loops and out-of-range endpoints dropped, one self loop added per node, duplicates keep their multiplicity -- 32 bits):
//     target-major  row_ptr [T+1], src [U], mult [U]     entries of a target in ascending source order
//     source-major  col_ptr [T+1], tgt [U], perm [U]     targets of a source ascending; perm = index of the target-major entry
// U <= cap = sum E + T entries; U stays on the device (row_ptr[T]).  Form of voxel.hip: a kernel writes 64-bit keys (target << 32 | source,
// one slot per listed edge and one per node for its self loop; a dropped edge gets the largest key), the caller sorts them (torch.sort),
// kernels mark the first slot of every run, compact the runs behind the caller's inclusive prefix sum of the marks, and repeat that for the
// transposed keys.  No step reads anything back to the host.
//
// The arithmetic is that of gat.hip's header:  e = leaky_relu(a_s[j] + a_d[i], 0.2), m = max over the target's entries,
// den = sum c exp(e - m) + 1e-16, alpha = c exp(e - m) / den, out[i] = sum alpha h[j] + bias.
//   logits    one wave per (node, head): a_s, a_d [T, heads]
//   forward   one wave per (target, head) walks the target's entries in chunks of 64: lanes span ENTRIES for max, sum and alpha; alpha and the
//             source id are then broadcast lane by lane (v_readlane) and lanes span CHANNELS for the aggregate -- a feature row is read as one
//             coalesced row (the rows of a graph and head are N C 4 bytes: L2)
//   backward  target-major pass, one wave per (target, head): g_ij = <dO[i], h[j]> per entry (lanes span channels, wave sum), then
//             d pre_ij = alpha_ij (g_ij - sum_j alpha_ij g_ij) lrelu'(pre_ij); c alpha and d pre are STORED per entry and head, d a_d[i] = sum_j d pre_ij
//             source-major pass, one wave per (source, head), over the transpose: d a_s[j] = sum_i d pre_ij and
//             dH[j] = sum_i c alpha_ij dO[i] + d a_s[j] att_src + d a_d[j] att_dst
//             d att_src = sum_j d a_s[j] h[j], d att_dst likewise: partial sums over blocks of 256 consecutive nodes, then a tree of fixed
//             shape over the partials (64 per group and level, each group in order)
// Every sum's order is fixed by the structure alone (lane l of a wave takes entries l, l + 64, ... in order, then the butterfly of wave_sum;
// an aggregate runs down its segment entry by entry), so a graph's outputs are the same bits alone or inside a batch and do not depend on
// the order in which the edge list names the edges.  A long segment is walked by its one wave (DESIGN: the star-graph figures).
#include "sga_common.h"

namespace {

constexpr int SP_THREADS = 256;
constexpr int SP_WAVES = SP_THREADS / 64;
constexpr int SP_CMAX = 256;                      // channels per head (CJ <= 4 slots per lane)
constexpr int SP_FOLD = 256;                      // nodes per partial sum of d att_src / d att_dst
constexpr int SP_TREE = 64;                       // partials one group of a fold level sums: ceil(log64(T / 256)) short levels, not one long walk
constexpr int SP_HEADS_MAX = 1 << 16;             // heads * channels <= 2^24 stays far inside int
constexpr long long SP_CAP_MAX = 0x7fffffffLL - 64;      // entries: the 64-entry chunk loops' `b += 64` cannot pass 2^31
constexpr float SP_SLOPE = 0.2f;
constexpr long long SP_DROPPED = 0x7fffffffffffffffLL;      // key of a slot that holds no entry: sorts behind every entry

__device__ __forceinline__ float sp_lrelu(float v) { return v > 0.f ? v : SP_SLOPE * v; }
__device__ __forceinline__ int sp_uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ int sp_lane_i(int v, int k) { return __builtin_amdgcn_readlane(v, k); }
__device__ __forceinline__ float sp_lane_f(float v, int k) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), k)); }
__device__ __forceinline__ int sp_hi(long long k) { return (int)(k >> 32); }
__device__ __forceinline__ int sp_lo(long long k) { return (int)(k & 0xffffffffLL); }

// ------------------------------------------------------------------------------------------------ structure
// slot s < E: listed edge s;  slot E + t: the self loop of node t
__global__ __launch_bounds__(SP_THREADS) void sp_keys_kernel(const long long* __restrict__ edges, const int* __restrict__ node_off,
                                                             const int* __restrict__ edge_off, int G, int T, int E, long long* __restrict__ keys) {
    const long long s = (long long)blockIdx.x * SP_THREADS + threadIdx.x;
    if (s >= (long long)E + T) return;
    long long key = SP_DROPPED;
    if (s >= E) {
        const long long t = s - E;
        key = (t << 32) | t;
    } else if (G > 0) {
        int lo = 0, hi = G;                        // the last graph g with edge_off[g] <= s
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (edge_off[mid] <= s) lo = mid; else hi = mid;
        }
        const int n0 = node_off[lo], N = node_off[lo + 1] - n0;
        if (edge_off[lo] <= s && s < edge_off[lo + 1] && n0 >= 0 && N > 0 && (long long)n0 + N <= T) {
            const long long sj = edges[2 * s], di = edges[2 * s + 1];
            if (sj != di && sj >= 0 && sj < N && di >= 0 && di < N) key = ((n0 + di) << 32) | (n0 + sj);
        }
    }
    keys[s] = key;
}

// head[s] = 1 where slot s of the sorted keys opens a run of equal keys (one entry)
__global__ __launch_bounds__(SP_THREADS) void sp_heads_kernel(const long long* __restrict__ sk, int cap, int* __restrict__ head) {
    const long long s = (long long)blockIdx.x * SP_THREADS + threadIdx.x;
    if (s >= cap) return;
    const long long k = sk[s];
    head[s] = (k != SP_DROPPED && (s == 0 || sk[s - 1] != k)) ? 1 : 0;
}

// incl = inclusive prefix sum of head.  The opening slot of entry u = incl[s] - 1 writes src[u], start[u] = s and the transposed key; the
// first entry of a target writes row_ptr (every target has its self loop, so every row_ptr[t] is written); the slot behind the last
// entry closes the structure: start[U] and row_ptr[T] = U.
__global__ __launch_bounds__(SP_THREADS) void sp_rows_kernel(const long long* __restrict__ sk, const int* __restrict__ incl, int cap, int T,
                                                             int* __restrict__ row_ptr, int* __restrict__ src, int* __restrict__ start,
                                                             long long* __restrict__ keys_t) {
    const long long s = (long long)blockIdx.x * SP_THREADS + threadIdx.x;
    if (s >= cap) return;
    const long long k = sk[s], prev = s ? sk[s - 1] : SP_DROPPED;
    if (k != SP_DROPPED) {
        if (s == 0 || prev != k) {
            const int u = incl[s] - 1, i = sp_hi(k), j = sp_lo(k);
            src[u] = j;
            start[u] = (int)s;
            keys_t[u] = ((long long)j << 32) | i;
            if (s == 0 || sp_hi(prev) != i) row_ptr[i] = u;
        }
        if (s == cap - 1) { start[incl[s]] = cap; row_ptr[T] = incl[s]; }
    } else if (s == 0 || prev != SP_DROPPED) {
        const int U = s ? incl[s - 1] : 0;
        start[U] = (int)s;
        row_ptr[T] = U;
    }
}

// mult[u] = length of run u; the slots behind U are cleared (their transposed key sorts last)
__global__ __launch_bounds__(SP_THREADS) void sp_mult_kernel(const int* __restrict__ start, const int* __restrict__ row_ptr, int cap, int T,
                                                             int* __restrict__ src, int* __restrict__ mult, long long* __restrict__ keys_t) {
    const long long u = (long long)blockIdx.x * SP_THREADS + threadIdx.x;
    if (u >= cap) return;
    if (u < row_ptr[T]) {
        mult[u] = start[u + 1] - start[u];
    } else {
        mult[u] = 0;
        src[u] = 0;
        keys_t[u] = SP_DROPPED;
    }
}

// the sorted transposed keys (source << 32 | target; all different) with the slot each came from
__global__ __launch_bounds__(SP_THREADS) void sp_cols_kernel(const long long* __restrict__ sk, const long long* __restrict__ order, int cap, int T,
                                                             int* __restrict__ col_ptr, int* __restrict__ tgt, int* __restrict__ perm) {
    const long long v = (long long)blockIdx.x * SP_THREADS + threadIdx.x;
    if (v >= cap) return;
    const long long k = sk[v], prev = v ? sk[v - 1] : SP_DROPPED;
    if (k != SP_DROPPED) {
        tgt[v] = sp_lo(k);
        perm[v] = (int)order[v];
        if (v == 0 || sp_hi(prev) != sp_hi(k)) col_ptr[sp_hi(k)] = (int)v;
        if (v == cap - 1) col_ptr[T] = cap;
    } else {
        tgt[v] = 0;
        perm[v] = 0;
        if (v == 0 || prev != SP_DROPPED) col_ptr[T] = (int)v;
    }
}

// ------------------------------------------------------------------------------------------------ attention
// lanes span the channels of a head in CJ slots (channel c = lane + 64 k); a lane past C reads channel C - 1 again with weight 0
template <int CJ>
struct SpChan {
    int cc[CJ];
    bool live[CJ];
    __device__ __forceinline__ SpChan(int lane, int C) {
#pragma unroll
        for (int q = 0; q < CJ; ++q) { cc[q] = min(lane + 64 * q, C - 1); live[q] = lane + 64 * q < C; }
    }
};

template <int CJ>
__global__ __launch_bounds__(SP_THREADS) void sp_logits_kernel(const float* __restrict__ H, const float* __restrict__ att_s,
                                                               const float* __restrict__ att_d, int T, int heads, int C,
                                                               float* __restrict__ as, float* __restrict__ ad) {
    const int lane = threadIdx.x & 63;
    const long long w = (long long)blockIdx.x * SP_WAVES + (threadIdx.x >> 6);
    if (w >= (long long)T * heads) return;
    const int hd = (int)(w % heads);
    const SpChan<CJ> ch(lane, C);
    const float* row = H + (size_t)w * C;          // (node, head) pairs are C apart: w * C = node * heads * C + hd * C
    float ps = 0.f, pd = 0.f;
#pragma unroll
    for (int q = 0; q < CJ; ++q) {
        const float h = row[ch.cc[q]];
        ps = fmaf(h, ch.live[q] ? att_s[hd * C + ch.cc[q]] : 0.f, ps);
        pd = fmaf(h, ch.live[q] ? att_d[hd * C + ch.cc[q]] : 0.f, pd);
    }
    const float vs = wave_sum(ps), vd = wave_sum(pd);
    if (lane == 0) { as[w] = vs; ad[w] = vd; }
}

// max and denominator of target i's softmax: lanes span the entries [beg, end)
__device__ __forceinline__ void sp_row_stats(const int* __restrict__ src, const int* __restrict__ mult, const float* __restrict__ as, int heads,
                                             int hd, float adi, int beg, int end, int lane, float& m, float& den) {
    float mloc = -INFINITY;
    for (int b = beg; b < end; b += 64) {
        const int u = b + lane;
        if (u < end) mloc = fmaxf(mloc, sp_lrelu(as[(size_t)src[u] * heads + hd] + adi));
    }
    m = wave_max(mloc);
    float sloc = 0.f;
    for (int b = beg; b < end; b += 64) {
        const int u = b + lane;
        if (u < end) sloc += (float)mult[u] * __expf(sp_lrelu(as[(size_t)src[u] * heads + hd] + adi) - m);
    }
    den = wave_sum(sloc) + 1e-16f;
}

template <int CJ>
__global__ __launch_bounds__(SP_THREADS) void sp_fwd_kernel(const float* __restrict__ H, const float* __restrict__ bias,
                                                            const int* __restrict__ row_ptr, const int* __restrict__ src,
                                                            const int* __restrict__ mult, const float* __restrict__ as,
                                                            const float* __restrict__ ad, float* __restrict__ out, int T, int heads, int C) {
    const int lane = threadIdx.x & 63;
    const long long w = (long long)blockIdx.x * SP_WAVES + (threadIdx.x >> 6);
    if (w >= (long long)T * heads) return;
    const int i = (int)(w / heads), hd = (int)(w % heads);
    const size_t HC = (size_t)heads * C;
    const int beg = sp_uniform(row_ptr[i]), end = sp_uniform(row_ptr[i + 1]);
    const float adi = ad[w];
    const SpChan<CJ> ch(lane, C);
    float m, den;
    sp_row_stats(src, mult, as, heads, hd, adi, beg, end, lane, m, den);
    const float* Hh = H + (size_t)hd * C;
    float acc[CJ];
#pragma unroll
    for (int q = 0; q < CJ; ++q) acc[q] = 0.f;
    for (int b = beg; b < end; b += 64) {
        const int u = b + lane, cnt = min(64, end - b);
        int j = 0;
        float a = 0.f;
        if (u < end) {
            j = src[u];
            a = (float)mult[u] * __expf(sp_lrelu(as[(size_t)j * heads + hd] + adi) - m) / den;
        }
#pragma unroll 4
        for (int k = 0; k < cnt; ++k) {
            const float ak = sp_lane_f(a, k);
            const float* row = Hh + (size_t)sp_lane_i(j, k) * HC;
#pragma unroll
            for (int q = 0; q < CJ; ++q) acc[q] = fmaf(ak, row[ch.cc[q]], acc[q]);
        }
    }
    float* o = out + (size_t)i * HC + (size_t)hd * C;
#pragma unroll
    for (int q = 0; q < CJ; ++q)
        if (ch.live[q]) o[ch.cc[q]] = acc[q] + bias[hd * C + ch.cc[q]];
}

// target-major backward pass.  wbuf / dpre: [heads][cap], entry-indexed; a lane reads back only what it stored itself.
template <int CJ>
__global__ __launch_bounds__(SP_THREADS) void sp_bwd_t_kernel(const float* __restrict__ H, const float* __restrict__ dO,
                                                              const int* __restrict__ row_ptr, const int* __restrict__ src,
                                                              const int* __restrict__ mult, const float* __restrict__ as,
                                                              const float* __restrict__ ad, float* wbuf, float* dpre,
                                                              float* __restrict__ dad, int T, int heads, int C, int cap) {
    const int lane = threadIdx.x & 63;
    const long long w = (long long)blockIdx.x * SP_WAVES + (threadIdx.x >> 6);
    if (w >= (long long)T * heads) return;
    const int i = (int)(w / heads), hd = (int)(w % heads);
    const size_t HC = (size_t)heads * C;
    const int beg = sp_uniform(row_ptr[i]), end = sp_uniform(row_ptr[i + 1]);
    const float adi = ad[w];
    const SpChan<CJ> ch(lane, C);
    float m, den;
    sp_row_stats(src, mult, as, heads, hd, adi, beg, end, lane, m, den);
    const float* Hh = H + (size_t)hd * C;
    float* wp = wbuf + (size_t)hd * cap;
    float* gp = dpre + (size_t)hd * cap;
    float dv[CJ];
#pragma unroll
    for (int q = 0; q < CJ; ++q) dv[q] = ch.live[q] ? dO[(size_t)i * HC + (size_t)hd * C + ch.cc[q]] : 0.f;
    float dot = 0.f;
    for (int b = beg; b < end; b += 64) {
        const int u = b + lane, cnt = min(64, end - b);
        int j = 0;
        float a = 0.f, g = 0.f;
        if (u < end) {
            j = src[u];
            a = (float)mult[u] * __expf(sp_lrelu(as[(size_t)j * heads + hd] + adi) - m) / den;
        }
#pragma unroll 4
        for (int k = 0; k < cnt; ++k) {
            const float* row = Hh + (size_t)sp_lane_i(j, k) * HC;
            float p = 0.f;
#pragma unroll
            for (int q = 0; q < CJ; ++q) p = fmaf(dv[q], row[ch.cc[q]], p);
            const float gk = wave_sum(p);
            if (lane == k) g = gk;
        }
        if (u < end) {
            wp[u] = a;
            gp[u] = g;
            dot = fmaf(a, g, dot);
        }
    }
    const float s = wave_sum(dot);
    float dsum = 0.f;
    for (int b = beg; b < end; b += 64) {
        const int u = b + lane;
        if (u < end) {
            const float pre = as[(size_t)src[u] * heads + hd] + adi;
            const float ds = wp[u] * (gp[u] - s) * (pre > 0.f ? 1.f : SP_SLOPE);
            gp[u] = ds;
            dsum += ds;
        }
    }
    const float dd = wave_sum(dsum);
    if (lane == 0) dad[w] = dd;
}

// source-major backward pass over the transpose
template <int CJ>
__global__ __launch_bounds__(SP_THREADS) void sp_bwd_s_kernel(const float* __restrict__ dO, const float* __restrict__ att_s,
                                                              const float* __restrict__ att_d, const int* __restrict__ col_ptr,
                                                              const int* __restrict__ tgt, const int* __restrict__ perm,
                                                              const float* __restrict__ wbuf, const float* __restrict__ dpre,
                                                              const float* __restrict__ dad, float* __restrict__ das,
                                                              float* __restrict__ dH, int T, int heads, int C, int cap) {
    const int lane = threadIdx.x & 63;
    const long long w = (long long)blockIdx.x * SP_WAVES + (threadIdx.x >> 6);
    if (w >= (long long)T * heads) return;
    const int j = (int)(w / heads), hd = (int)(w % heads);
    const size_t HC = (size_t)heads * C;
    const int beg = sp_uniform(col_ptr[j]), end = sp_uniform(col_ptr[j + 1]);
    const SpChan<CJ> ch(lane, C);
    const float* wp = wbuf + (size_t)hd * cap;
    const float* gp = dpre + (size_t)hd * cap;
    const float* Dh = dO + (size_t)hd * C;
    float acc[CJ];
#pragma unroll
    for (int q = 0; q < CJ; ++q) acc[q] = 0.f;
    float dloc = 0.f;
    for (int b = beg; b < end; b += 64) {
        const int v = b + lane, cnt = min(64, end - b);
        int i = 0;
        float a = 0.f;
        if (v < end) {
            const int pe = perm[v];
            i = tgt[v];
            a = wp[pe];
            dloc += gp[pe];
        }
#pragma unroll 4
        for (int k = 0; k < cnt; ++k) {
            const float ak = sp_lane_f(a, k);
            const float* row = Dh + (size_t)sp_lane_i(i, k) * HC;
#pragma unroll
            for (int q = 0; q < CJ; ++q) acc[q] = fmaf(ak, row[ch.cc[q]], acc[q]);
        }
    }
    const float dasj = wave_sum(dloc), dadj = dad[w];
    if (lane == 0) das[w] = dasj;
    float* o = dH + (size_t)j * HC + (size_t)hd * C;
#pragma unroll
    for (int q = 0; q < CJ; ++q)
        if (ch.live[q]) o[ch.cc[q]] = acc[q] + dasj * att_s[hd * C + ch.cc[q]] + dadj * att_d[hd * C + ch.cc[q]];
}

// d att, stage 1: part[p][0][col] = sum over the nodes j of block p (in order) of d a_s[j] h[j][col], part[p][1][col] with d a_d
__global__ __launch_bounds__(SP_THREADS) void sp_datt_part_kernel(const float* __restrict__ H, const float* __restrict__ das,
                                                                  const float* __restrict__ dad, int T, int heads, int C,
                                                                  float* __restrict__ part) {
    const int HC = heads * C, col = blockIdx.y * SP_THREADS + threadIdx.x, p = blockIdx.x;
    if (col >= HC) return;
    const int hd = col / C, j1 = (int)min((long long)T, ((long long)p + 1) * SP_FOLD);
    float gs = 0.f, gd = 0.f;
    for (int j = p * SP_FOLD; j < j1; ++j) {
        const float h = H[(size_t)j * HC + col];
        gs = fmaf(das[(size_t)j * heads + hd], h, gs);
        gd = fmaf(dad[(size_t)j * heads + hd], h, gd);
    }
    part[((size_t)p * 2 + 0) * HC + col] = gs;
    part[((size_t)p * 2 + 1) * HC + col] = gd;
}

// stage 2, one level of a tree of fixed shape: group g = blockIdx.x folds the partials [g SP_TREE, (g + 1) SP_TREE) of `in` in order into
// partial g of `out`; the level that is left with one group writes d att_src / d att_dst themselves (out == nullptr)
__global__ __launch_bounds__(SP_THREADS) void sp_datt_fold_kernel(const float* __restrict__ in, int P, int HC, float* __restrict__ out,
                                                                  float* __restrict__ d_att_s, float* __restrict__ d_att_d) {
    const int col = blockIdx.y * SP_THREADS + threadIdx.x, g = blockIdx.x;
    if (col >= HC) return;
    const int p1 = min(P, (g + 1) * SP_TREE);
    float gs = 0.f, gd = 0.f;
    for (int p = g * SP_TREE; p < p1; ++p) {
        gs += in[((size_t)p * 2 + 0) * HC + col];
        gd += in[((size_t)p * 2 + 1) * HC + col];
    }
    if (out) {
        out[((size_t)g * 2 + 0) * HC + col] = gs;
        out[((size_t)g * 2 + 1) * HC + col] = gd;
    } else {
        d_att_s[col] = gs;
        d_att_d[col] = gd;
    }
}

// ------------------------------------------------------------------------------------------------ host
int sp_check_hc(int heads, int channels, const char* who) {
    if (heads < 1 || heads > SP_HEADS_MAX) { sga_set_error("%s: heads %d outside 1 .. %d", who, heads, SP_HEADS_MAX); return SGA_ERR_ARG; }
    if (channels < 1 || channels > SP_CMAX) {
        sga_set_error("%s: channels %d outside 1 .. %d per head", who, channels, SP_CMAX);
        return SGA_ERR_ARG;
    }
    return SGA_OK;
}

inline unsigned sp_blocks(long long n) { return (unsigned)((n + SP_THREADS - 1) / SP_THREADS); }
inline unsigned sp_wave_blocks(int T, int heads) { return (unsigned)(((long long)T * heads + SP_WAVES - 1) / SP_WAVES); }
inline int sp_parts(int T) { return (int)(((long long)T + SP_FOLD - 1) / SP_FOLD); }
// partials of every level of the fold tree together (the last level's single group goes to the outputs; its slot is simply not used)
inline size_t sp_parts_all(int T) {
    size_t all = 0;
    for (int P = sp_parts(T); ; P = (P + SP_TREE - 1) / SP_TREE) {
        all += (size_t)P;
        if (P <= 1) return all;
    }
}

// float counts of the workspace's parts, in order: a_s, a_d [, d a_d, d a_s, c alpha, d pre, d att partials]
inline size_t sp_ws_floats(int T, int cap, int heads, int channels, bool bwd) {
    const size_t th = (size_t)T * heads;
    if (!bwd) return 2 * th;
    return 4 * th + 2 * (size_t)heads * cap + sp_parts_all(T) * 2 * (size_t)heads * channels;
}

#define SP_CJ(KERNEL, GRID, STREAM, ...)                                                                                   \
    switch ((channels + 63) / 64) {                                                                                        \
        case 1: hipLaunchKernelGGL(KERNEL<1>, GRID, dim3(SP_THREADS), 0, STREAM, __VA_ARGS__); break;                      \
        case 2: hipLaunchKernelGGL(KERNEL<2>, GRID, dim3(SP_THREADS), 0, STREAM, __VA_ARGS__); break;                      \
        case 3: hipLaunchKernelGGL(KERNEL<3>, GRID, dim3(SP_THREADS), 0, STREAM, __VA_ARGS__); break;                      \
        default: hipLaunchKernelGGL(KERNEL<4>, GRID, dim3(SP_THREADS), 0, STREAM, __VA_ARGS__); break;                     \
    }

}  // namespace

extern "C" int sga_gat_sp_capacity(int T, int E) {
    if (T < 0 || E < 0) { sga_set_error("sga_gat_sp_capacity: negative size"); return -1; }
    if ((long long)T + E > SP_CAP_MAX) {
        sga_set_error("sga_gat_sp_capacity: %d nodes + %d listed edges: the entry count must stay below 2^31 - 64", T, E);
        return -1;
    }
    return T + E;
}

extern "C" size_t sga_gat_sp_build_workspace_bytes(int cap) { return cap < 0 ? 0 : ((size_t)cap + 1) * sizeof(int); }

extern "C" size_t sga_gat_sp_workspace_bytes(int T, int cap, int heads, int channels, int bwd) {
    if (sp_check_hc(heads, channels, "sga_gat_sp_workspace_bytes")) return 0;
    if (T < 0 || cap < 0) { sga_set_error("sga_gat_sp_workspace_bytes: negative size"); return 0; }
    if (cap > SP_CAP_MAX) { sga_set_error("sga_gat_sp_workspace_bytes: capacity %d: must stay below 2^31 - 64", cap); return 0; }
    return sp_ws_floats(T, cap, heads, channels, bwd != 0) * sizeof(float);
}

extern "C" int sga_gat_sp_keys(const int64_t* edges, const int32_t* node_off, const int32_t* edge_off, int G, int T, int E, int64_t* keys,
                               void* stream) {
    SGA_CHECK_ARG(G >= 0 && T >= 0 && E >= 0, "sga_gat_sp_keys: negative size");
    SGA_CHECK_ARG(sga_gat_sp_capacity(T, E) >= 0, "sga_gat_sp_keys: %d nodes + %d listed edges: the entry count must stay below 2^31 - 64", T, E);
    const int cap = T + E;
    if (cap == 0) return SGA_OK;
    SGA_CHECK_ARG(keys && (E == 0 || (edges && node_off && edge_off)), "sga_gat_sp_keys: null pointer");
    hipLaunchKernelGGL(sp_keys_kernel, dim3(sp_blocks(cap)), dim3(SP_THREADS), 0, static_cast<hipStream_t>(stream),
                       reinterpret_cast<const long long*>(edges), node_off, edge_off, G, T, E, reinterpret_cast<long long*>(keys));
    SGA_CHECK_LAUNCH("sga_gat_sp_keys");
    return SGA_OK;
}

extern "C" int sga_gat_sp_heads(const int64_t* sorted_keys, int cap, int32_t* head, void* stream) {
    SGA_CHECK_ARG(cap >= 0, "sga_gat_sp_heads: negative size");
    SGA_CHECK_ARG(cap <= SP_CAP_MAX, "sga_gat_sp_heads: capacity %d: must stay below 2^31 - 64", cap);
    if (cap == 0) return SGA_OK;
    SGA_CHECK_ARG(sorted_keys && head, "sga_gat_sp_heads: null pointer");
    hipLaunchKernelGGL(sp_heads_kernel, dim3(sp_blocks(cap)), dim3(SP_THREADS), 0, static_cast<hipStream_t>(stream),
                       reinterpret_cast<const long long*>(sorted_keys), cap, head);
    SGA_CHECK_LAUNCH("sga_gat_sp_heads");
    return SGA_OK;
}

extern "C" int sga_gat_sp_rows(const int64_t* sorted_keys, const int32_t* head_incl, int cap, int T, int32_t* row_ptr, int32_t* src,
                               int32_t* mult, int64_t* keys_t, void* workspace, size_t ws_bytes, void* stream) {
    SGA_CHECK_ARG(cap >= 0 && T >= 0, "sga_gat_sp_rows: negative size");
    SGA_CHECK_ARG(cap <= SP_CAP_MAX, "sga_gat_sp_rows: capacity %d: must stay below 2^31 - 64", cap);
    SGA_CHECK_ARG(T <= cap, "sga_gat_sp_rows: capacity %d below the %d self loops", cap, T);
    SGA_CHECK_ARG(row_ptr, "sga_gat_sp_rows: null pointer");
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (cap == 0) return sga_zero("sga_gat_sp_rows", row_ptr, sizeof(int), s);
    SGA_CHECK_ARG(sorted_keys && head_incl && src && mult && keys_t && workspace, "sga_gat_sp_rows: null pointer");
    if (ws_bytes < sga_gat_sp_build_workspace_bytes(cap)) {
        sga_set_error("sga_gat_sp_rows: workspace of %zu bytes, %zu needed", ws_bytes, sga_gat_sp_build_workspace_bytes(cap));
        return SGA_ERR_WORKSPACE;
    }
    int* start = static_cast<int*>(workspace);
    hipLaunchKernelGGL(sp_rows_kernel, dim3(sp_blocks(cap)), dim3(SP_THREADS), 0, s, reinterpret_cast<const long long*>(sorted_keys), head_incl,
                       cap, T, row_ptr, src, start, reinterpret_cast<long long*>(keys_t));
    hipLaunchKernelGGL(sp_mult_kernel, dim3(sp_blocks(cap)), dim3(SP_THREADS), 0, s, start, row_ptr, cap, T, src, mult,
                       reinterpret_cast<long long*>(keys_t));
    SGA_CHECK_LAUNCH("sga_gat_sp_rows");
    return SGA_OK;
}

extern "C" int sga_gat_sp_cols(const int64_t* sorted_keys_t, const int64_t* order_t, int cap, int T, int32_t* col_ptr, int32_t* tgt,
                               int32_t* perm, void* stream) {
    SGA_CHECK_ARG(cap >= 0 && T >= 0, "sga_gat_sp_cols: negative size");
    SGA_CHECK_ARG(cap <= SP_CAP_MAX, "sga_gat_sp_cols: capacity %d: must stay below 2^31 - 64", cap);
    SGA_CHECK_ARG(T <= cap, "sga_gat_sp_cols: capacity %d below the %d self loops", cap, T);
    SGA_CHECK_ARG(col_ptr, "sga_gat_sp_cols: null pointer");
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (cap == 0) return sga_zero("sga_gat_sp_cols", col_ptr, sizeof(int), s);
    SGA_CHECK_ARG(sorted_keys_t && order_t && tgt && perm, "sga_gat_sp_cols: null pointer");
    hipLaunchKernelGGL(sp_cols_kernel, dim3(sp_blocks(cap)), dim3(SP_THREADS), 0, s, reinterpret_cast<const long long*>(sorted_keys_t),
                       reinterpret_cast<const long long*>(order_t), cap, T, col_ptr, tgt, perm);
    SGA_CHECK_LAUNCH("sga_gat_sp_cols");
    return SGA_OK;
}

extern "C" int sga_gat_sp_fwd(const float* H, int heads, int channels, const float* att_src, const float* att_dst, const float* bias,
                              const int32_t* row_ptr, const int32_t* src, const int32_t* mult, int T, float* out, void* workspace,
                              size_t ws_bytes, void* stream) {
    int rc = sp_check_hc(heads, channels, "sga_gat_sp_fwd");
    if (rc) return rc;
    SGA_CHECK_ARG(T >= 0, "sga_gat_sp_fwd: negative size");
    SGA_CHECK_ARG((long long)T * heads <= 0x7fffffffLL, "sga_gat_sp_fwd: %d nodes x %d heads: must stay below 2^31", T, heads);
    if (T == 0) return SGA_OK;
    SGA_CHECK_ARG(H && att_src && att_dst && bias && row_ptr && src && mult && out && workspace, "sga_gat_sp_fwd: null pointer");
    const size_t need = sp_ws_floats(T, 0, heads, channels, false) * sizeof(float);
    if (ws_bytes < need) {
        sga_set_error("sga_gat_sp_fwd: workspace of %zu bytes, %zu needed", ws_bytes, need);
        return SGA_ERR_WORKSPACE;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    float* as = static_cast<float*>(workspace);
    float* ad = as + (size_t)T * heads;
    const dim3 grid(sp_wave_blocks(T, heads));
    SP_CJ(sp_logits_kernel, grid, s, H, att_src, att_dst, T, heads, channels, as, ad)
    SP_CJ(sp_fwd_kernel, grid, s, H, bias, row_ptr, src, mult, as, ad, out, T, heads, channels)
    SGA_CHECK_LAUNCH("sga_gat_sp_fwd");
    return SGA_OK;
}

extern "C" int sga_gat_sp_bwd(const float* H, const float* dO, int heads, int channels, const float* att_src, const float* att_dst,
                              const int32_t* row_ptr, const int32_t* src, const int32_t* mult, const int32_t* col_ptr, const int32_t* tgt,
                              const int32_t* perm, int T, int cap, float* dH, float* d_att_src, float* d_att_dst, void* workspace,
                              size_t ws_bytes, void* stream) {
    int rc = sp_check_hc(heads, channels, "sga_gat_sp_bwd");
    if (rc) return rc;
    SGA_CHECK_ARG(T >= 0 && cap >= 0, "sga_gat_sp_bwd: negative size");
    SGA_CHECK_ARG(cap <= SP_CAP_MAX, "sga_gat_sp_bwd: capacity %d: must stay below 2^31 - 64", cap);
    SGA_CHECK_ARG(T <= cap, "sga_gat_sp_bwd: capacity %d below the %d self loops", cap, T);
    SGA_CHECK_ARG((long long)T * heads <= 0x7fffffffLL, "sga_gat_sp_bwd: %d nodes x %d heads: must stay below 2^31", T, heads);
    SGA_CHECK_ARG(d_att_src && d_att_dst, "sga_gat_sp_bwd: null pointer");
    SGA_CHECK_ARG(T == 0 || (H && dO && att_src && att_dst && row_ptr && src && mult && col_ptr && tgt && perm && dH && workspace),
                  "sga_gat_sp_bwd: null pointer");
    const size_t need = sp_ws_floats(T, cap, heads, channels, true) * sizeof(float);
    if (T > 0 && ws_bytes < need) {
        sga_set_error("sga_gat_sp_bwd: workspace of %zu bytes, %zu needed", ws_bytes, need);
        return SGA_ERR_WORKSPACE;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int HC = heads * channels;
    if (T == 0) {
        rc = sga_zero("sga_gat_sp_bwd", d_att_src, HC * sizeof(float), s);
        return rc ? rc : sga_zero("sga_gat_sp_bwd", d_att_dst, HC * sizeof(float), s);
    }
    const size_t th = (size_t)T * heads;
    float* as = static_cast<float*>(workspace);
    float* ad = as + th;
    float* dad = ad + th;
    float* das = dad + th;
    float* wbuf = das + th;
    float* dpre = wbuf + (size_t)heads * cap;
    float* part = dpre + (size_t)heads * cap;          // every level of the fold tree, one behind the other
    const int P = sp_parts(T);
    const dim3 grid(sp_wave_blocks(T, heads));
    SP_CJ(sp_logits_kernel, grid, s, H, att_src, att_dst, T, heads, channels, as, ad)
    SP_CJ(sp_bwd_t_kernel, grid, s, H, dO, row_ptr, src, mult, as, ad, wbuf, dpre, dad, T, heads, channels, cap)
    SP_CJ(sp_bwd_s_kernel, grid, s, dO, att_src, att_dst, col_ptr, tgt, perm, wbuf, dpre, dad, das, dH, T, heads, channels, cap)
    hipLaunchKernelGGL(sp_datt_part_kernel, dim3(P, (HC + SP_THREADS - 1) / SP_THREADS), dim3(SP_THREADS), 0, s, H, das, dad, T, heads, channels, part);
    for (int Pin = P; ; ) {                                         // the fold tree: levels of SP_TREE partials per group, down to one group
        const int Pout = (Pin + SP_TREE - 1) / SP_TREE;
        float* nxt = part + (size_t)Pin * 2 * HC;
        hipLaunchKernelGGL(sp_datt_fold_kernel, dim3(Pout, (HC + SP_THREADS - 1) / SP_THREADS), dim3(SP_THREADS), 0, s, part, Pin, HC,
                           Pout > 1 ? nxt : nullptr, d_att_src, d_att_dst);
        if (Pout <= 1) break;
        part = nxt;
        Pin = Pout;
    }
    SGA_CHECK_LAUNCH("sga_gat_sp_bwd");
    return SGA_OK;
}
