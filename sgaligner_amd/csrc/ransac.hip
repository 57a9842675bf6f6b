// Batched RANSAC rigid registration from point correspondences, fp64 (the estimator of src/engine/registration_evaluator.py:129-208:
// pygcransac.findRigidTransform at min_iters == max_iters and spatial_coherence_weight == 0, i.e. a fixed number of three-point
// hypotheses, each scored against every correspondence, then least-squares refits on the inliers).
//
// Jobs (one [n, 6] correspondence array = source xyz | reference xyz, and its sample triples) share one packed upload.  The samples are
// an INPUT: nothing here draws random numbers, so the output is a pure function of the arguments.
//
//   ransac_hyp_kernel     one lane per hypothesis: the least-squares rigid fit of its three pairs -> model [12][total_hyp] (R row-major | t).
//                         A repeated or out-of-range index, or a non-finite result, stores NaN: such a model passes no point test.
//   ransac_score_kernel   the hot path.  A workgroup of 256 lanes holds RS_HPL models per lane in registers (12 fp64 each) and walks one chunk
//                         of the job's rows through LDS tiles (structure of arrays, every lane reads the same address: broadcast).  15 fp64
//                         operations per (hypothesis, row); the per-lane count is an integer register.  Per-chunk counts go to a
//                         [n_chunks, total_hyp] int32 workspace ...
//   ransac_fold_kernel    ... that this kernel sums in ascending chunk order -> hyp_count.
//   ransac_select_kernel  per job: the lowest index among the hypotheses with the maximal count (an invalid one has count 0 and a NaN model;
//                         a best count below 3 is "no model", status 1).
//   ransac_accum_kernel   moments of the inliers of the candidate model (count, sum s, sum r, sum s r^T about the job's first row), per
//                         1024-row slice: lanes in row order, a wave butterfly, the four waves in order.  ransac_step_kernel folds the slices
//                         in ascending order (the second stage; no floating-point atomics anywhere), accepts the candidate when its count
//                         is >= the current one, and fits the next candidate from the accepted model's moments.
//   ransac_mask_kernel    the final model's inlier mask.
//
// Every point test in every kernel is the same sequence of explicit fma / mul / sub (ransac_inlier), so a count and the mask that
// belongs to it can never disagree.
#include <math.h>

#include "pair_jobs.h"
#include "rigid_solver.h"

namespace {

constexpr int RS_THREADS = 256;
constexpr int RS_HPL = 4;                          // hypotheses per lane: 4 x 12 fp64 = 96 VGPRs of models
constexpr int RS_HTILE = RS_THREADS * RS_HPL;      // hypotheses per workgroup
constexpr int RS_STILE = 256;                      // rows per LDS tile (6 x 256 x 8 B = 12 KiB)
constexpr int RS_RPL = 4;                          // rows per lane in the refit / mask kernels
constexpr int RS_RCHUNK = RS_THREADS * RS_RPL;     // rows per workgroup there
constexpr int RS_MAX_ROUNDS = 64;

struct RSState {            // per job, in the workspace
    double cur[12];         // accepted model: R row-major, then t
    double cand[12];        // the model the next accum pass measures
    int cur_count, stopped, pad0, pad1;
};

// |R s + t - r|^2 <= thr2, every operation explicit.  A NaN model fails the test.
__host__ __device__ __forceinline__ bool ransac_inlier(const double* m, double sx, double sy, double sz, double rx, double ry, double rz,
                                                       double thr2) {
    const double dx = fma(m[0], sx, fma(m[1], sy, fma(m[2], sz, m[9]))) - rx;
    const double dy = fma(m[3], sx, fma(m[4], sy, fma(m[5], sz, m[10]))) - ry;
    const double dz = fma(m[6], sx, fma(m[7], sy, fma(m[8], sz, m[11]))) - rz;
    return fma(dz, dz, fma(dy, dy, dx * dx)) <= thr2;
}

__global__ __launch_bounds__(RS_THREADS) void ransac_hyp_kernel(const double* __restrict__ corr, const int* __restrict__ off, int total_rows,
                                                                const int* __restrict__ samples, const int* __restrict__ hoff, int total_hyp,
                                                                int g_tiles, double* __restrict__ model) {
    const int job = blockIdx.x / g_tiles;
    const int h = (blockIdx.x % g_tiles) * RS_THREADS + threadIdx.x;
    const SgaHypJob J = sga_hyp_job(off, total_rows, hoff, total_hyp, job);
    if (!J.ok || h >= J.nh) return;
    const size_t g = (size_t)J.h0 + h;
    const int ia = samples[3 * g], ib = samples[3 * g + 1], ic = samples[3 * g + 2];
    double out[12];
#pragma unroll
    for (int a = 0; a < 12; ++a) out[a] = NAN;
    const bool valid = ia >= 0 && ia < J.n && ib >= 0 && ib < J.n && ic >= 0 && ic < J.n && ia != ib && ia != ic && ib != ic;
    if (valid) {
        const double* C = corr + (size_t)J.o0 * 6;
        double pa[6], S[15];
#pragma unroll
        for (int a = 0; a < 6; ++a) pa[a] = C[(size_t)ia * 6 + a];
#pragma unroll
        for (int a = 0; a < 15; ++a) S[a] = 0.0;
#pragma unroll
        for (int k = 0; k < 2; ++k) {                       // the first pair is the pivot: its own moments are zero
            const double* row = C + (size_t)(k == 0 ? ib : ic) * 6;
            double d[6];
#pragma unroll
            for (int a = 0; a < 6; ++a) d[a] = row[a] - pa[a];
#pragma unroll
            for (int a = 0; a < 6; ++a) S[a] += d[a];
#pragma unroll
            for (int a = 0; a < 3; ++a)
#pragma unroll
                for (int b = 0; b < 3; ++b) S[6 + 3 * a + b] = fma(d[a], d[3 + b], S[6 + 3 * a + b]);
        }
        rigid_from_moments(3.0, S, pa, pa + 3, out);
    }
#pragma unroll
    for (int a = 0; a < 12; ++a) model[(size_t)a * total_hyp + g] = out[a];
}

__global__ __launch_bounds__(RS_THREADS) void ransac_score_kernel(const double* __restrict__ corr, const int* __restrict__ off, int total_rows,
                                                                  const int* __restrict__ hoff, int total_hyp,
                                                                  const double* __restrict__ model, double thr2, int h_tiles, int n_chunks,
                                                                  int chunk, int* __restrict__ ws_cnt) {
    __shared__ double tile[6][RS_STILE];
    const int tid = threadIdx.x;
    int b = blockIdx.x;
    const int ht = b % h_tiles;
    b /= h_tiles;
    const int c = b % n_chunks, job = b / n_chunks;
    const SgaHypJob J = sga_hyp_job(off, total_rows, hoff, total_hyp, job);
    if (!J.ok) return;
    const int hb = ht * RS_HTILE;
    if (hb >= J.nh) return;
    const int my_chunks = J.n <= chunk ? 1 : (int)(((long long)J.n + chunk - 1) / chunk);      // no rows: one pass that writes zeros
    if (c >= my_chunks) return;
    const int c0 = c * chunk, c1 = (int)min((long long)J.n, (long long)c0 + chunk);           // c < my_chunks: c * chunk < n

    double m[RS_HPL][12];
    int cnt[RS_HPL];
#pragma unroll
    for (int k = 0; k < RS_HPL; ++k) {
        const int h = hb + k * RS_THREADS + tid;
        const bool ok = h < J.nh;
#pragma unroll
        for (int a = 0; a < 12; ++a) m[k][a] = ok ? model[(size_t)a * total_hyp + J.h0 + h] : NAN;
        cnt[k] = 0;
    }
    const double* C = corr + (size_t)J.o0 * 6;
    for (int t0 = c0; t0 < c1; t0 += RS_STILE) {
        const int rows = min(RS_STILE, c1 - t0);
        __syncthreads();                                       // the previous tile has been consumed by every wave
        for (int e = tid; e < rows * 6; e += RS_THREADS) tile[e % 6][e / 6] = C[(size_t)t0 * 6 + e];
        __syncthreads();
#pragma unroll 2
        for (int j = 0; j < rows; ++j) {
            const double sx = tile[0][j], sy = tile[1][j], sz = tile[2][j], rx = tile[3][j], ry = tile[4][j], rz = tile[5][j];
#pragma unroll
            for (int k = 0; k < RS_HPL; ++k) cnt[k] += ransac_inlier(m[k], sx, sy, sz, rx, ry, rz, thr2) ? 1 : 0;
        }
    }
#pragma unroll
    for (int k = 0; k < RS_HPL; ++k) {
        const int h = hb + k * RS_THREADS + tid;
        if (h < J.nh) ws_cnt[(size_t)c * total_hyp + J.h0 + h] = cnt[k];
    }
}

__global__ __launch_bounds__(RS_THREADS) void ransac_fold_kernel(const int* __restrict__ off, int total_rows, const int* __restrict__ hoff,
                                                                 int total_hyp, int g_tiles, int n_chunks, int chunk,
                                                                 const int* __restrict__ ws_cnt, int* __restrict__ hyp_count) {
    const int job = blockIdx.x / g_tiles;
    const int h = (blockIdx.x % g_tiles) * RS_THREADS + threadIdx.x;
    const SgaHypJob J = sga_hyp_job(off, total_rows, hoff, total_hyp, job);
    if (!J.ok || h >= J.nh) return;
    const int my_chunks = J.n <= chunk ? 1 : (int)min((long long)n_chunks, ((long long)J.n + chunk - 1) / chunk);   // never past what was written
    int s = 0;
#pragma unroll 8
    for (int c = 0; c < my_chunks; ++c) s += ws_cnt[(size_t)c * total_hyp + J.h0 + h];
    hyp_count[(size_t)J.h0 + h] = s;
}

__global__ __launch_bounds__(RS_THREADS) void ransac_select_kernel(const int* __restrict__ off, int total_rows, const int* __restrict__ hoff,
                                                                   int total_hyp, const int* __restrict__ hyp_count,
                                                                   const double* __restrict__ model, RSState* __restrict__ state,
                                                                   int* __restrict__ best_hyp, int* __restrict__ status) {
    __shared__ int s_cnt[RS_THREADS], s_idx[RS_THREADS];
    const int tid = threadIdx.x, job = blockIdx.x;
    const SgaHypJob J = sga_hyp_job(off, total_rows, hoff, total_hyp, job);
    int bc = -1, bi = 0x7fffffff;
    if (J.ok)
        for (int h = tid; h < J.nh; h += RS_THREADS) {
            const int c = hyp_count[(size_t)J.h0 + h];
            if (c > bc) { bc = c; bi = h; }                    // ascending walk, strict >: the lowest index of a maximum stays
        }
    s_cnt[tid] = bc;
    s_idx[tid] = bi;
    __syncthreads();
    for (int w = RS_THREADS / 2; w > 0; w >>= 1) {
        if (tid < w) {
            const int c2 = s_cnt[tid + w], i2 = s_idx[tid + w];
            if (c2 > s_cnt[tid] || (c2 == s_cnt[tid] && i2 < s_idx[tid])) { s_cnt[tid] = c2; s_idx[tid] = i2; }
        }
        __syncthreads();
    }
    if (tid != 0) return;
    RSState* st = state + job;
    const bool found = J.ok && J.n >= 3 && s_cnt[0] >= 3;
    for (int a = 0; a < 12; ++a) {
        const double v = found ? model[(size_t)a * total_hyp + J.h0 + s_idx[0]] : ((a == 0 || a == 4 || a == 8) ? 1.0 : 0.0);
        st->cur[a] = v;
        st->cand[a] = v;
    }
    st->cur_count = found ? s_cnt[0] : 0;
    st->stopped = found ? 0 : 1;
    best_hyp[job] = found ? s_idx[0] : -1;
    status[job] = found ? 0 : 1;
}

// Moments of the inliers of state[job].cand over one RS_RCHUNK slice of the job's rows -> partials[job][slice][16] (slot 15: the count).
__global__ __launch_bounds__(RS_THREADS) void ransac_accum_kernel(const double* __restrict__ corr, const int* __restrict__ off, int total_rows,
                                                                  const int* __restrict__ hoff, int total_hyp,
                                                                  const RSState* __restrict__ state, double thr2, int r_chunks,
                                                                  double* __restrict__ partials) {
    __shared__ double red[RS_THREADS / 64][16];
    const int tid = threadIdx.x, job = blockIdx.x / r_chunks, c = blockIdx.x % r_chunks;
    const SgaHypJob J = sga_hyp_job(off, total_rows, hoff, total_hyp, job);
    if (!J.ok || state[job].stopped) return;
    const int c0 = c * RS_RCHUNK;                              // c < r_chunks <= ceil(max_rows / RS_RCHUNK): no overflow
    if (c0 >= J.n) return;
    double m[12], piv[6], acc[16];
    const double* C = corr + (size_t)J.o0 * 6;
#pragma unroll
    for (int a = 0; a < 12; ++a) m[a] = state[job].cand[a];
#pragma unroll
    for (int a = 0; a < 6; ++a) piv[a] = C[a];
#pragma unroll
    for (int a = 0; a < 16; ++a) acc[a] = 0.0;
#pragma unroll
    for (int k = 0; k < RS_RPL; ++k) {
        const int i = c0 + k * RS_THREADS + tid;
        if (i >= J.n) continue;
        double p[6];
#pragma unroll
        for (int a = 0; a < 6; ++a) p[a] = C[(size_t)i * 6 + a];
        if (!ransac_inlier(m, p[0], p[1], p[2], p[3], p[4], p[5], thr2)) continue;
#pragma unroll
        for (int a = 0; a < 6; ++a) { p[a] -= piv[a]; acc[a] += p[a]; }
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int b2 = 0; b2 < 3; ++b2) acc[6 + 3 * a + b2] = fma(p[a], p[3 + b2], acc[6 + 3 * a + b2]);
        acc[15] += 1.0;
    }
#pragma unroll
    for (int a = 0; a < 16; ++a) acc[a] = wave_sum_d(acc[a]);
    if ((tid & 63) == 0) {
#pragma unroll
        for (int a = 0; a < 16; ++a) red[tid >> 6][a] = acc[a];
    }
    __syncthreads();
    if (tid < 16) {
        double s = red[0][tid];
        for (int w = 1; w < RS_THREADS / 64; ++w) s += red[w][tid];
        partials[((size_t)job * r_chunks + c) * 16 + tid] = s;
    }
}

// Round `round` of `rounds`: fold the candidate's slices, accept or stop, fit the next candidate; the last round writes the outputs.
__global__ __launch_bounds__(64) void ransac_step_kernel(const double* __restrict__ corr, const int* __restrict__ off, int total_rows,
                                                         const int* __restrict__ hoff, int total_hyp, RSState* __restrict__ state,
                                                         int r_chunks, const double* __restrict__ partials, int round, int rounds,
                                                         const int* __restrict__ status, double* __restrict__ transform,
                                                         int* __restrict__ inlier_count) {
    __shared__ double S[16];
    const int tid = threadIdx.x, job = blockIdx.x;
    const SgaHypJob J = sga_hyp_job(off, total_rows, hoff, total_hyp, job);
    RSState* st = state + job;
    const bool live = J.ok && !st->stopped;                    // uniform over the workgroup
    if (live && tid < 16) {
        const int my = (int)min((long long)r_chunks, ((long long)J.n + RS_RCHUNK - 1) / RS_RCHUNK);
        double s = 0.0;
        for (int c = 0; c < my; ++c) s += partials[((size_t)job * r_chunks + c) * 16 + tid];      // ascending: a fixed order
        S[tid] = s;
    }
    __syncthreads();
    if (tid != 0) return;
    if (live) {
        const int cnt = (int)S[15];
        if (round == 0 || cnt >= st->cur_count) {
            for (int a = 0; a < 12; ++a) st->cur[a] = st->cand[a];
            st->cur_count = cnt;
            if (round < rounds) {
                double fit[12];
                const double* C = corr + (size_t)J.o0 * 6;
                double piv[6];
                for (int a = 0; a < 6; ++a) piv[a] = C[a];
                if (cnt >= 3 && rigid_from_moments((double)cnt, S, piv, piv + 3, fit)) {
                    for (int a = 0; a < 12; ++a) st->cand[a] = fit[a];
                } else {
                    st->stopped = 1;
                }
            }
        } else {
            st->stopped = 1;
        }
    }
    if (round == rounds) {
        const bool ok = J.ok && status[job] == 0;
        double* T = transform + (size_t)job * 16;
        for (int a = 0; a < 3; ++a) {
            for (int b2 = 0; b2 < 3; ++b2) T[4 * a + b2] = ok ? st->cur[3 * a + b2] : (a == b2 ? 1.0 : 0.0);
            T[4 * a + 3] = ok ? st->cur[9 + a] : 0.0;
            T[12 + a] = 0.0;
        }
        T[15] = 1.0;
        inlier_count[job] = ok ? st->cur_count : 0;
    }
}

__global__ __launch_bounds__(RS_THREADS) void ransac_mask_kernel(const double* __restrict__ corr, const int* __restrict__ off, int total_rows,
                                                                 const int* __restrict__ hoff, int total_hyp,
                                                                 const RSState* __restrict__ state, const int* __restrict__ status,
                                                                 double thr2, int r_chunks, unsigned char* __restrict__ mask) {
    const int tid = threadIdx.x, job = blockIdx.x / r_chunks, c = blockIdx.x % r_chunks;
    const SgaHypJob J = sga_hyp_job(off, total_rows, hoff, total_hyp, job);
    if (!J.ok) return;
    const int c0 = c * RS_RCHUNK;
    if (c0 >= J.n) return;
    const bool ok = status[job] == 0;
    double m[12];
#pragma unroll
    for (int a = 0; a < 12; ++a) m[a] = state[job].cur[a];
    const double* C = corr + (size_t)J.o0 * 6;
#pragma unroll
    for (int k = 0; k < RS_RPL; ++k) {
        const int i = c0 + k * RS_THREADS + tid;
        if (i >= J.n) continue;
        const double* p = C + (size_t)i * 6;
        mask[(size_t)J.o0 + i] = (ok && ransac_inlier(m, p[0], p[1], p[2], p[3], p[4], p[5], thr2)) ? 1 : 0;
    }
}

struct RSLayout { size_t model, state, partials, counts, total; };

inline RSLayout rs_layout(int n_jobs, int total_hyp, int max_rows, int chunk) {
    RSLayout L;
    L.model = 0;
    L.state = L.model + (size_t)12 * total_hyp * sizeof(double);
    L.partials = L.state + (size_t)n_jobs * sizeof(RSState);
    L.counts = L.partials + (size_t)n_jobs * sga_chunks(max_rows, RS_RCHUNK) * 16 * sizeof(double);
    L.total = L.counts + (((size_t)sga_chunks(max_rows, chunk) * total_hyp * sizeof(int32_t) + 7) & ~(size_t)7);
    return L;
}

}  // namespace

static_assert(sizeof(RSState) % 8 == 0, "RSState keeps the arrays after it 8-byte aligned");

extern "C" size_t sga_ransac_workspace_bytes(int n_jobs, int total_hyp, int max_rows, int chunk) {
    if (n_jobs <= 0 || total_hyp < 0 || max_rows < 0 || chunk <= 0) return 0;
    return rs_layout(n_jobs, total_hyp, max_rows, chunk).total;
}

extern "C" int sga_ransac_rigid(const double* corr, const int32_t* offsets, int n_jobs, int total_rows, const int32_t* samples,
                                const int32_t* hyp_offsets, int total_hyp, int max_rows, int max_hyp, int chunk,
                                const int32_t* offsets_host, const int32_t* hyp_offsets_host, double threshold, int refine_rounds,
                                double* transform, int32_t* inlier_count, int32_t* best_hyp, int32_t* status, unsigned char* inlier_mask,
                                int32_t* hyp_count, void* workspace, size_t workspace_bytes, void* stream) {
    SGA_CHECK_ARG(n_jobs >= 0 && total_rows >= 0 && total_hyp >= 0 && max_rows >= 0 && max_hyp >= 0,
                  "sga_ransac_rigid: negative count (n_jobs %d, total_rows %d, total_hyp %d, max_rows %d, max_hyp %d)", n_jobs, total_rows,
                  total_hyp, max_rows, max_hyp);
    SGA_CHECK_ARG(chunk >= 1, "sga_ransac_rigid: chunk must be >= 1 (got %d)", chunk);
    SGA_CHECK_ARG(refine_rounds >= -1 && refine_rounds <= RS_MAX_ROUNDS, "sga_ransac_rigid: refine_rounds must be in [-1, %d] (got %d)",
                  RS_MAX_ROUNDS, refine_rounds);
    SGA_CHECK_ARG(threshold >= 0.0 && isfinite(threshold), "sga_ransac_rigid: threshold must be finite and >= 0 (got %g)", threshold);
    SGA_CHECK_ARG(max_rows <= total_rows && max_hyp <= total_hyp, "sga_ransac_rigid: max_rows %d / max_hyp %d exceed total_rows %d / total_hyp %d",
                  max_rows, max_hyp, total_rows, total_hyp);
    if (n_jobs == 0) return SGA_OK;                                                              // nothing to write
    SGA_CHECK_ARG(offsets && hyp_offsets && transform && inlier_count && best_hyp && status, "sga_ransac_rigid: null pointer");
    SGA_CHECK_ARG((corr && inlier_mask) || total_rows == 0, "sga_ransac_rigid: null pointer (corr / inlier_mask with total_rows %d)", total_rows);
    SGA_CHECK_ARG((samples && hyp_count) || total_hyp == 0, "sga_ransac_rigid: null pointer (samples / hyp_count with total_hyp %d)", total_hyp);
    SGA_CHECK_ARG(sga_aligned(8, corr, transform, workspace) && sga_aligned(4, offsets, samples, hyp_offsets, inlier_count, best_hyp, status, hyp_count),
                  "sga_ransac_rigid: misaligned pointer (fp64 arrays need 8 bytes, int32 arrays 4)");
    const SgaPrefix OFFSETS{"offsets", "decrease", "job", "total_rows", "rows", "max_rows"};
    const SgaPrefix HYP_OFFSETS{"hyp_offsets", "decrease", "job", "total_hyp", "hypotheses", "max_hyp"};
    if (int rc = sga_check_prefix("sga_ransac_rigid", OFFSETS, offsets_host, n_jobs, total_rows, max_rows)) return rc;
    if (int rc = sga_check_prefix("sga_ransac_rigid", HYP_OFFSETS, hyp_offsets_host, n_jobs, total_hyp, max_hyp)) return rc;
    const long n_chunks = sga_chunks(max_rows, chunk), r_chunks = sga_chunks(max_rows, RS_RCHUNK);
    const long h_tiles = ((long)max_hyp + RS_HTILE - 1) / RS_HTILE, g_tiles = ((long)max_hyp + RS_THREADS - 1) / RS_THREADS;
    const char* advice = "raise chunk or split the job list";
    if (int rc = sga_check_grid("sga_ransac_rigid", h_tiles, n_chunks, n_jobs, advice)) return rc;
    if (int rc = sga_check_grid("sga_ransac_rigid", g_tiles, 1, n_jobs, advice)) return rc;
    if (int rc = sga_check_grid("sga_ransac_rigid", r_chunks, 1, n_jobs, advice)) return rc;
    const RSLayout L = rs_layout(n_jobs, total_hyp, max_rows, chunk);
    if (int rc = sga_check_workspace("sga_ransac_rigid", L.total, workspace, workspace_bytes)) return rc;     // L.total > 0: a state per job
    hipStream_t s = static_cast<hipStream_t>(stream);
    char* ws = static_cast<char*>(workspace);
    double* model = reinterpret_cast<double*>(ws + L.model);
    RSState* state = reinterpret_cast<RSState*>(ws + L.state);
    double* partials = reinterpret_cast<double*>(ws + L.partials);
    int* ws_cnt = reinterpret_cast<int*>(ws + L.counts);
    const double thr2 = threshold * threshold;
    if (h_tiles > 0) {
        hipLaunchKernelGGL(ransac_hyp_kernel, dim3((unsigned)(g_tiles * n_jobs)), dim3(RS_THREADS), 0, s, corr, offsets, total_rows, samples,
                           hyp_offsets, total_hyp, (int)g_tiles, model);
        hipLaunchKernelGGL(ransac_score_kernel, dim3((unsigned)(h_tiles * n_chunks * n_jobs)), dim3(RS_THREADS), 0, s, corr, offsets, total_rows,
                           hyp_offsets, total_hyp, model, thr2, (int)h_tiles, (int)n_chunks, chunk, ws_cnt);
        hipLaunchKernelGGL(ransac_fold_kernel, dim3((unsigned)(g_tiles * n_jobs)), dim3(RS_THREADS), 0, s, offsets, total_rows, hyp_offsets,
                           total_hyp, (int)g_tiles, (int)n_chunks, chunk, ws_cnt, hyp_count);
    }
    if (refine_rounds < 0) {                                                                     // scoring only: hyp_count and nothing else
        SGA_CHECK_LAUNCH("sga_ransac_rigid");
        return SGA_OK;
    }
    hipLaunchKernelGGL(ransac_select_kernel, dim3((unsigned)n_jobs), dim3(RS_THREADS), 0, s, offsets, total_rows, hyp_offsets, total_hyp, hyp_count,
                       model, state, best_hyp, status);
    for (int round = 0; round <= refine_rounds; ++round) {
        hipLaunchKernelGGL(ransac_accum_kernel, dim3((unsigned)(r_chunks * n_jobs)), dim3(RS_THREADS), 0, s, corr, offsets, total_rows, hyp_offsets,
                           total_hyp, state, thr2, (int)r_chunks, partials);
        hipLaunchKernelGGL(ransac_step_kernel, dim3((unsigned)n_jobs), dim3(64), 0, s, corr, offsets, total_rows, hyp_offsets, total_hyp, state,
                           (int)r_chunks, partials, round, refine_rounds, status, transform, inlier_count);
    }
    if (total_rows > 0)
        hipLaunchKernelGGL(ransac_mask_kernel, dim3((unsigned)(r_chunks * n_jobs)), dim3(RS_THREADS), 0, s, corr, offsets, total_rows, hyp_offsets,
                           total_hyp, state, status, thr2, (int)r_chunks, inlier_mask);
    SGA_CHECK_LAUNCH("sga_ransac_rigid");
    return SGA_OK;
}
