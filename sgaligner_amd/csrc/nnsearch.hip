// Batched exact nearest-neighbour search in 3-D, fp64 (the point-cloud geometry on both sides of the path).
//
// Replaces utils/point_cloud.py:136-147 (get_nearest_neighbor: cKDTree(s).query(q, k=1)), the radius search of
// utils/point_cloud.py:91-103 (compute_pcl_overlap, r = 1e-7: "is the nearest target point within r") and the one-query-
// per-vertex loop of utils/registration.py:107-129 (nn_correspondence).  Brute force: every (query, support) pair is
// evaluated, so the answer is exact and independent of any tree.
//
// Arithmetic contract: d2 = (dx*dx + dy*dy) + dz*dz with dx = q.x - s.x ..., every operation rounded on its own (the
// explicit __d*_rn forms AND -ffp-contract=off for this file, _build.FILE_FLAGS), dist = correctly rounded sqrt(d2).  With
// this order the distances are bit-identical to cKDTree's.  Ties: the LOWEST support index among the exact minima (strict <
// while the support is walked in ascending order; chunks are merged in ascending order with strict <) -- numpy.argmin's rule.
//
// Jobs (query cloud, support cloud) share one packed upload.  nn_kernel: a workgroup of 256 lanes holds NN_QPL queries per
// lane in registers and walks one chunk of the support through LDS tiles (SoA, every lane reads the same address: broadcast).
// About 11 fp64 VALU operations per pair against three LDS reads per NN_QPL pairs: fp64-VALU-issue bound.  A job whose support
// fits one chunk writes its result directly; larger supports are split over chunks across workgroups into a
// [n_chunks, total_queries] partial workspace that nn_merge_kernel folds in fixed order.  No atomics anywhere: the output is
// a pure function of the input.
#include <math.h>

#include "pair_jobs.h"

namespace {

constexpr int NN_THREADS = 256;
constexpr int NN_QPL = 4;                         // queries per lane (6 VGPRs of coordinates + 3 of running best each)
constexpr int NN_QTILE = NN_THREADS * NN_QPL;     // queries per workgroup
constexpr int NN_STILE = 512;                     // support points per LDS tile (12 KiB)

__global__ __launch_bounds__(NN_THREADS) void nn_kernel(const double* __restrict__ pts, const int* __restrict__ off, int n_clouds,
                                                        int total_points, const int* __restrict__ pairs, int n_pairs,
                                                        const int* __restrict__ out_off, int total_queries, int q_tiles,
                                                        int n_chunks, int chunk, int squared, double* __restrict__ out_d,
                                                        int* __restrict__ out_i, double* __restrict__ ws_d, int* __restrict__ ws_i) {
    __shared__ double sx[NN_STILE], sy[NN_STILE], sz[NN_STILE];
    const int tid = threadIdx.x;
    int b = blockIdx.x;
    const int qt = b % q_tiles;
    b /= q_tiles;
    const int c = b % n_chunks, job = b / n_chunks;
    const SgaPairJob J = sga_pair_job(off, n_clouds, total_points, pairs, n_pairs, out_off, total_queries, job);
    if (!J.ok) return;
    const int qb = qt * NN_QTILE;
    if (qb >= J.nq) return;
    const int my_chunks = sga_chunks(J.ns, chunk);     // empty support: one pass that writes (+inf, -1)
    if (c >= my_chunks) return;
    const int c0 = c * chunk, c1 = (int)min((long long)J.ns, (long long)c0 + chunk);     // c < my_chunks: c * chunk < ns

    const double* Q = pts + (size_t)J.q0 * 3;
    const double* S = pts + (size_t)J.s0 * 3;
    double qx[NN_QPL], qy[NN_QPL], qz[NN_QPL], bd[NN_QPL];
    int bi[NN_QPL];
#pragma unroll
    for (int k = 0; k < NN_QPL; ++k) {
        const int i = qb + k * NN_THREADS + tid;
        const bool ok = i < J.nq;
        qx[k] = ok ? Q[(size_t)i * 3 + 0] : 0.0;
        qy[k] = ok ? Q[(size_t)i * 3 + 1] : 0.0;
        qz[k] = ok ? Q[(size_t)i * 3 + 2] : 0.0;
        bd[k] = INFINITY;
        bi[k] = -1;
    }
    for (int t0 = c0; t0 < c1; t0 += NN_STILE) {
        const int m = min(NN_STILE, c1 - t0);
        __syncthreads();                                       // the previous tile has been consumed by every wave
        for (int j = tid; j < m; j += NN_THREADS) {
            sx[j] = S[(size_t)(t0 + j) * 3 + 0];
            sy[j] = S[(size_t)(t0 + j) * 3 + 1];
            sz[j] = S[(size_t)(t0 + j) * 3 + 2];
        }
        __syncthreads();
#pragma unroll 4
        for (int j = 0; j < m; ++j) {
            const double x = sx[j], y = sy[j], z = sz[j];
            const int idx = t0 + j;
#pragma unroll
            for (int k = 0; k < NN_QPL; ++k) {
                const double dx = __dsub_rn(qx[k], x), dy = __dsub_rn(qy[k], y), dz = __dsub_rn(qz[k], z);
                const double d2 = __dadd_rn(__dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)), __dmul_rn(dz, dz));
                if (d2 < bd[k]) { bd[k] = d2; bi[k] = idx; }   // strict: the first (lowest) index of a minimum stays
            }
        }
    }
    const bool direct = my_chunks == 1;
#pragma unroll
    for (int k = 0; k < NN_QPL; ++k) {
        const int i = qb + k * NN_THREADS + tid;
        if (i >= J.nq) continue;
        if (direct) {
            out_d[(size_t)J.oo + i] = squared ? bd[k] : __dsqrt_rn(bd[k]);
            out_i[(size_t)J.oo + i] = bi[k];
        } else {
            const size_t w = (size_t)c * total_queries + J.oo + i;
            ws_d[w] = bd[k];
            ws_i[w] = bi[k];
        }
    }
}

// Jobs that were split: fold the chunks' partial minima in ascending chunk order (strict <, so equal minima keep the lower index).
__global__ __launch_bounds__(NN_THREADS) void nn_merge_kernel(const int* __restrict__ off, int n_clouds, int total_points,
                                                              const int* __restrict__ pairs, int n_pairs, const int* __restrict__ out_off,
                                                              int total_queries, int m_tiles, int n_chunks, int chunk, int squared,
                                                              double* __restrict__ out_d, int* __restrict__ out_i,
                                                              const double* __restrict__ ws_d, const int* __restrict__ ws_i) {
    const int job = blockIdx.x / m_tiles;
    const int i = (blockIdx.x % m_tiles) * NN_THREADS + threadIdx.x;
    const SgaPairJob J = sga_pair_job(off, n_clouds, total_points, pairs, n_pairs, out_off, total_queries, job);
    if (!J.ok || J.ns <= chunk || i >= J.nq) return;
    const int my_chunks = min(n_chunks, sga_chunks(J.ns, chunk));   // never past what nn_kernel wrote
    double bd = INFINITY;
    int bi = -1;
    for (int c = 0; c < my_chunks; ++c) {
        const size_t w = (size_t)c * total_queries + J.oo + i;
        const double d = ws_d[w];
        if (d < bd) { bd = d; bi = ws_i[w]; }
    }
    out_d[(size_t)J.oo + i] = squared ? bd : __dsqrt_rn(bd);
    out_i[(size_t)J.oo + i] = bi;
}

}  // namespace

extern "C" size_t sga_nn_workspace_bytes(int total_queries, int max_support, int chunk) {
    if (total_queries <= 0 || max_support <= 0 || chunk <= 0) return 0;
    const long nc = sga_chunks(max_support, chunk);
    return nc <= 1 ? 0 : (size_t)nc * (size_t)total_queries * (sizeof(double) + sizeof(int32_t));
}

extern "C" int sga_nn_search(const double* pts, const int32_t* offsets, int n_clouds, int total_points, const int32_t* pairs, int n_pairs,
                             const int32_t* out_offsets, int total_queries, int max_queries, int max_support, int chunk,
                             const int32_t* offsets_host, const int32_t* pairs_host, int squared, double* out_dist,
                             int32_t* out_idx, void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "sga_nn_search";
    SGA_CHECK_ARG(n_clouds >= 0 && total_points >= 0 && n_pairs >= 0 && total_queries >= 0 && max_queries >= 0 && max_support >= 0,
                  "sga_nn_search: negative count (n_clouds %d, total_points %d, n_pairs %d, total_queries %d, max_queries %d, max_support %d)",
                  n_clouds, total_points, n_pairs, total_queries, max_queries, max_support);
    if (int rc = sga_check_chunked(who, chunk, max_queries, total_queries)) return rc;
    if (n_pairs == 0 || total_queries == 0 || max_queries == 0) return SGA_OK;               // nothing to write
    SGA_CHECK_ARG(offsets && pairs && out_offsets && out_dist && out_idx, "sga_nn_search: null pointer");
    SGA_CHECK_ARG(pts || total_points == 0, "sga_nn_search: null point array");
    SGA_CHECK_ARG(sga_aligned(8, pts, out_dist, workspace) && sga_aligned(4, offsets, pairs, out_offsets, out_idx),
                  "sga_nn_search: misaligned pointer (fp64 arrays need 8 bytes, int32 arrays 4)");
    const SgaPrefix OFFSETS{"offsets", "decrease", "cloud", "total_points", nullptr, nullptr};
    if (int rc = sga_check_prefix(who, OFFSETS, offsets_host, n_clouds, total_points, SGA_ANY)) return rc;
    if (int rc = sga_check_pairs(who, "cloud", pairs_host, n_pairs, offsets_host, n_clouds, max_queries, max_support)) return rc;
    const long n_chunks = sga_chunks(max_support, chunk);
    const long q_tiles = ((long)max_queries + NN_QTILE - 1) / NN_QTILE, m_tiles = ((long)max_queries + NN_THREADS - 1) / NN_THREADS;
    if (int rc = sga_check_grid(who, q_tiles, n_chunks, n_pairs, "raise chunk or split the job list")) return rc;
    if (int rc = sga_check_grid(who, m_tiles, 1, n_pairs, "raise chunk or split the job list")) return rc;
    const size_t need = sga_nn_workspace_bytes(total_queries, max_support, chunk);
    if (int rc = sga_check_workspace(who, need, workspace, workspace_bytes)) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    double* ws_d = static_cast<double*>(workspace);
    int* ws_i = need ? reinterpret_cast<int*>(ws_d + (size_t)n_chunks * total_queries) : nullptr;
    hipLaunchKernelGGL(nn_kernel, dim3((unsigned)(q_tiles * n_chunks * n_pairs)), dim3(NN_THREADS), 0, s, pts, offsets, n_clouds, total_points,
                       pairs, n_pairs, out_offsets, total_queries, (int)q_tiles, (int)n_chunks, chunk, squared, out_dist, out_idx, ws_d, ws_i);
    if (need)
        hipLaunchKernelGGL(nn_merge_kernel, dim3((unsigned)(m_tiles * n_pairs)), dim3(NN_THREADS), 0, s, offsets, n_clouds, total_points, pairs,
                           n_pairs, out_offsets, total_queries, (int)m_tiles, (int)n_chunks, chunk, squared, out_dist, out_idx, ws_d, ws_i);
    SGA_CHECK_LAUNCH("sga_nn_search");
    return SGA_OK;
}
