// Feature-matching RANSAC scored geometrically (Open3D's registration_ransac_based_on_feature_matching): every validated hypothesis is
// judged by evaluate_registration -- a nearest-neighbour search of ALL moved source points in the reference cloud -- not by the feature
// correspondences it was drawn from.  The contract written in include/sgaligner_hip.h IS the definition; tests/ransac_geo_ref.py restates
// it in numpy.  Two entries:
//
//   sga_ransac_models          one lane per hypothesis: ransac.hip's three-point model (rigid_solver.h's solver, the same validity rules) as an
//                              output of its own, [total_hyp, 12] row-major [R | t], with a valid flag and the largest residual of the three
//                              sampled rows (Open3D's distance checker reads it).  The residual is taken with the search's arithmetic below,
//                              so numpy recomputes it bit for bit from the downloaded model.
//   sga_score_transforms_grid  the hot path: per job (query cloud, support cloud, transform) the number of queries that sga_nn_search_grid
//                              would give a partner, and the sum of their d2 -- without ever writing the 12 B per query of that search.
//                              geo_score_kernel searches and folds a slice; geo_fold_kernel adds the slices.
//
// Every fp64 operation is rounded on its own (explicit __d*_rn forms in the search, -ffp-contract=off for this file); the solver's explicit
// fma() calls are rigid_solver.h's.  No atomics: both entries are pure functions of their inputs.  Every id, offset and index read from a device
// array is re-checked: a bad one makes the workgroup do nothing (or skip that candidate), never read or write out of bounds.
//
// THE SEARCH is icp_nn_grid_kernel's walk, written out again (gs_search; its helpers are wave_search.h's): one wave per query, the clamp of
// the cell coordinate in fp64, the blocks |k - c|inf <= R for R = 1, 2, 4, 8, 16 around the clamped cell, every (kx, ky) row one range of sorted
// positions found by two binary searches, the stop rule with its 2^-40 margins, and the walk of the whole support for a query that stays
// undecided, has a non-finite moved coordinate or meets a support without a grid.  The proof that the stop rule is exact, also for a centre
// outside the box, stands at the head of icp.hip and is not repeated; nothing in it depends on what is done with the result.
//
// THE FOLD is fixed, after icp_accum_kernel.  A slice is GS_SLICE = 1024 query rows counted from the job's first row; one workgroup of four
// waves per (job, slice).  Wave w owns rows w, w + 4, w + 8, ... of the slice (so that a short cloud still feeds all four waves) and goes
// through them in ascending order, one search each, adding the d2 of a found partner to a running sum that every lane holds alike (the butterfly leaves the wave's best in all 64 lanes) and
// counting it.  Then the four waves in order (LDS), then geo_fold_kernel the slices in ascending order.  So sum_d2 of a job is
//     fold over slices c ascending ( fold over waves w = 0..3 ( fold over the wave's rows ascending ) )
// with every fold starting at +0.0: the same bits in two calls, for a job alone or in a batch, and for every cell size -- the grid decides
// how much of the support is looked at, never what comes out.
#include "pair_jobs.h"
#include "rigid_solver.h"
#include "wave_search.h"

namespace {

// ---- models ----------------------------------------------------------------------------------------------------------------------------------
constexpr int GM_THREADS = 256;

// A value that every lane of the wave holds alike, as a scalar: the compiler then keeps it and what is derived from it in SGPRs.
__device__ __forceinline__ double gs_uniform(double v) {
    const long long b = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_readfirstlane((int)b), hi = __builtin_amdgcn_readfirstlane((int)(b >> 32));
    return __longlong_as_double((long long)(((unsigned long long)(unsigned)hi << 32) | (unsigned)lo));
}

// |R s + t - r|^2 of one corr row under model m, in the search's arithmetic: sga_move_point, then (dx dx + dy dy) + dz dz.
__device__ __forceinline__ double gm_resid2(const double* m, const double* row) {
    const double dx = __dsub_rn(sga_move_point(m, 0, row[0], row[1], row[2]), row[3]);
    const double dy = __dsub_rn(sga_move_point(m, 1, row[0], row[1], row[2]), row[4]);
    const double dz = __dsub_rn(sga_move_point(m, 2, row[0], row[1], row[2]), row[5]);
    return __dadd_rn(__dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)), __dmul_rn(dz, dz));
}

__global__ __launch_bounds__(GM_THREADS) void geo_models_kernel(const double* __restrict__ corr, const int* __restrict__ off, int total_rows,
                                                                const int* __restrict__ samples, const int* __restrict__ hoff, int total_hyp,
                                                                int g_tiles, double* __restrict__ models, int* __restrict__ valid,
                                                                double* __restrict__ resid2) {
    const int job = blockIdx.x / g_tiles;
    const int h = (blockIdx.x % g_tiles) * GM_THREADS + threadIdx.x;
    const SgaHypJob J = sga_hyp_job(off, total_rows, hoff, total_hyp, job);
    if (!J.ok || h >= J.nh) return;
    const size_t g = (size_t)J.h0 + h;
    const int ia = samples[3 * g], ib = samples[3 * g + 1], ic = samples[3 * g + 2];
    double out[12];
#pragma unroll
    for (int a = 0; a < 12; ++a) out[a] = NAN;
    bool ok = ia >= 0 && ia < J.n && ib >= 0 && ib < J.n && ic >= 0 && ic < J.n && ia != ib && ia != ic && ib != ic;
    double worst = INFINITY;
    if (ok) {
        const double* C = corr + (size_t)J.o0 * 6;
        double pa[6], pb[6], pc[6], S[15];
#pragma unroll
        for (int a = 0; a < 6; ++a) {
            pa[a] = C[(size_t)ia * 6 + a];
            pb[a] = C[(size_t)ib * 6 + a];
            pc[a] = C[(size_t)ic * 6 + a];
        }
#pragma unroll
        for (int a = 0; a < 15; ++a) S[a] = 0.0;
#pragma unroll
        for (int k = 0; k < 2; ++k) {                       // the first pair is the pivot: its own moments are zero
            double d[6];
#pragma unroll
            for (int a = 0; a < 6; ++a) d[a] = (k == 0 ? pb[a] : pc[a]) - pa[a];
#pragma unroll
            for (int a = 0; a < 6; ++a) S[a] += d[a];
#pragma unroll
            for (int a = 0; a < 3; ++a)
#pragma unroll
                for (int b = 0; b < 3; ++b) S[6 + 3 * a + b] = fma(d[a], d[3 + b], S[6 + 3 * a + b]);
        }
        ok = rigid_from_moments(3.0, S, pa, pa + 3, out);
        if (ok) {
            const double ra = gm_resid2(out, pa), rb = gm_resid2(out, pb), rc = gm_resid2(out, pc);
            ok = ra == ra && rb == rb && rc == rc;          // a NaN residual (an overflow on the way): no model
            worst = fmax(fmax(ra, rb), rc);
        }
        if (!ok) {
            worst = INFINITY;
#pragma unroll
            for (int a = 0; a < 12; ++a) out[a] = NAN;
        }
    }
#pragma unroll
    for (int a = 0; a < 12; ++a) models[g * 12 + a] = out[a];
    valid[g] = ok ? 1 : 0;
    resid2[g] = worst;
}

// ---- the fused search and fold -----------------------------------------------------------------------------------------------------------------
constexpr int GS_THREADS = 256;
constexpr int GS_WAVES = 4;
constexpr int GS_SLICE = 1024;                     // query rows per workgroup, counted from the job's first row (icp.hip's IC_SLICE)

struct GSPartial { double sum; long long count; };

// What the wave needs to know about the job's support, read once.
struct GSSupport {
    const double* P;          // the support's rows
    const int* ord;           // its slice of `order`
    const long long* sk;      // its slice of sorted_keys
    const double* geo;        // LDS: the support's origin (3), its cell edge, r2 -- read where they are used, as vector values, and never
                              // held across the search: as scalars they are 10 SGPRs too many
    int ns, s0, sc, dm[3];
    bool grid;                // the support has a usable grid
};

__device__ __forceinline__ bool gs_uniform(bool v) { return __builtin_amdgcn_readfirstlane(v ? 1 : 0) != 0; }

// icp_nn_grid_kernel's search of one moved query (qx, qy, qz), by the whole wave: the best (d2, j) in every lane, (+inf, INT_MAX) without one.
__device__ __forceinline__ void gs_search(const GSSupport& U, double qx, double qy, double qz, int lane, int* __restrict__ rs,
                                          int* __restrict__ rx, double& bd, int& bj) {
    int kc[3];
    bool use_grid = U.grid && isfinite(qx) && isfinite(qy) && isfinite(qz);
    const double r2 = U.geo[4];
    const long long cloud_bits = (long long)U.sc << 48;
    {
        const double h = U.geo[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const double qa = a == 0 ? qx : (a == 1 ? qy : qz);
            double t = floor(__ddiv_rn(__dsub_rn(qa, U.geo[a]), h));
            use_grid = use_grid && U.dm[a] > 0 && t == t;                    // no kept point, or a NaN: the whole walk
            t = fmin(fmax(t, 0.0), (double)(U.dm[a] > 0 ? U.dm[a] - 1 : 0)); // clamped in fp64: t may be -inf, +inf or beyond any int
            kc[a] = __builtin_amdgcn_readfirstlane(t == t ? (int)t : 0);
        }
        use_grid = gs_uniform(use_grid);
    }
    bd = INFINITY;
    bj = INT_MAX;
    bool decided = false;
    if (use_grid) {
#pragma unroll 1
        for (int R = 1; R <= GRID_MAX_R && !decided; R *= 2) {
            const int x0 = max(kc[0] - R, 0), y0 = max(kc[1] - R, 0), z0 = max(kc[2] - R, 0);
            const int x1 = min(kc[0] + R, U.dm[0] - 1), y1 = min(kc[1] + R, U.dm[1] - 1), z1 = min(kc[2] + R, U.dm[2] - 1);
            const int ny = y1 - y0 + 1, rows = (x1 - x0 + 1) * ny;       // at most 33 x 33
#pragma unroll 1
            for (int rb = 0; rb < rows; rb += 64) {
                const int r = rb + lane;
                int start = 0, len = 0;
                if (r < rows) {
                    const long long rowkey = cloud_bits | ((long long)(x0 + r / ny) << 32) | ((long long)(y0 + r % ny) << 16);
                    start = sga_lower_bound(U.sk, U.ns, rowkey | (long long)z0);
                    len = sga_lower_bound(U.sk, U.ns, (rowkey | (long long)z1) + 1) - start;
                    if (len < 0) len = 0;
                }
                const int incl = wave_incl_scan(len, lane);
                const int total_len = __shfl(incl, 63, 64);
                sga_wave_sync();                                          // the previous batch's table has been read by every lane
                rs[lane] = start;
                rx[lane] = incl - len;
                sga_wave_sync();
#pragma unroll 1
                for (int u0 = 0; u0 < total_len; u0 += 64) {
                    const bool inb = u0 + lane < total_len;
                    const int u = inb ? u0 + lane : total_len - 1;
                    int lo = 0;                                          // the LAST row whose exclusive prefix is <= u: rows of length 0 are passed over
#pragma unroll
                    for (int step = 32; step > 0; step >>= 1)
                        if (rx[lo + step] <= u) lo += step;              // lo + step <= 63
                    const int t = rs[lo] + (u - rx[lo]);
                    const bool tin = t >= 0 && t < U.ns;
                    const int i = tin ? U.ord[t] : U.s0;
                    const bool jin = tin && i >= U.s0 && i - U.s0 < U.ns;
                    const int j = jin ? i - U.s0 : 0;
                    const double d2 = sga_point_d2(qx, qy, qz, U.P + (size_t)j * 3);        // total_len > 0: the support has a row 0
                    sga_nn_offer(r2, d2, j, inb && jin, bd, bj);
                }
            }
            sga_wave_best(bd, bj);
            if (x0 == 0 && y0 == 0 && z0 == 0 && x1 == U.dm[0] - 1 && y1 == U.dm[1] - 1 && z1 == U.dm[2] - 1) { decided = true; break; }   // the whole box
            // the stop rule: see the head of icp.hip
            const double bound = fmin(r2, bd), h = U.geo[3];
            double g = INFINITY;
            bool ok = true;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const double o = U.geo[a], qa = a == 0 ? qx : (a == 1 ? qy : qz);
                const double scale = __dadd_rn(fmax(fabs(o), fabs(qa)), __dmul_rn((double)(kc[a] + R + 1), h));
                double gap = INFINITY;
                if (kc[a] - R > 0) gap = __dsub_rn(qa, __dadd_rn(o, __dmul_rn((double)(kc[a] - R), h)));
                if (kc[a] + R < U.dm[a] - 1) {
                    const double up = __dsub_rn(__dadd_rn(o, __dmul_rn((double)(kc[a] + R + 1), h)), qa);
                    ok = ok && up == up && gap == gap;
                    gap = fmin(gap, up);
                }
                const double ga = __dsub_rn(gap, __dmul_rn(GRID_EPS, scale));
                ok = ok && ga > 0.0;                                     // a NaN is not > 0
                g = fmin(g, ga);
            }
            if (gs_uniform(ok && g > 0.0 && __dmul_rn(__dmul_rn(g, g), 1.0 - GRID_EPS) > bound)) decided = true;
        }
    }
    if (!decided) {                                                      // the whole support in original order, as nn_kernel looks at it
        bd = INFINITY;
        bj = INT_MAX;
        for (int j = lane; j < U.ns; j += 64) sga_nn_offer(r2, sga_point_d2(qx, qy, qz, U.P + (size_t)j * 3), j, true, bd, bj);
        sga_wave_best(bd, bj);
    }
}

__global__ __launch_bounds__(GS_THREADS) void geo_score_kernel(const double* __restrict__ pts, const int* __restrict__ off, int n_clouds,
                                                               int total_points, const int* __restrict__ pairs, int n_pairs, int slices,
                                                               const double* __restrict__ cell, const double* __restrict__ origin,
                                                               const int* __restrict__ dims, const int* __restrict__ status,
                                                               const int* __restrict__ order, const long long* __restrict__ sorted_keys,
                                                               const double* __restrict__ transforms, const int* __restrict__ live, double r2,
                                                               GSPartial* __restrict__ partials) {
    __shared__ int row_start[GS_WAVES][64], row_excl[GS_WAVES][64];
    __shared__ double red_sum[GS_WAVES], s_m[12], s_geo[5];
    __shared__ int red_cnt[GS_WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int job = blockIdx.x / slices, c = blockIdx.x % slices;
    const SgaCloudPair J = sga_cloud_pair(off, n_clouds, total_points, pairs, n_pairs, job);
    if (!J.ok) return;                                                   // every exit before the barrier is uniform over the workgroup
    if (live && live[job] == 0) return;
    const int c0 = c * GS_SLICE;                                         // c < slices <= ceil(max_queries / GS_SLICE): no overflow
    if (c0 >= J.nq) return;

    // The job's transform waits in LDS and is read again for every query: held in registers it is 24 SGPRs that live across the whole
    // search, which then spills.  A value read from LDS is a vector value; the moved query is made a scalar again (gs_uniform), so that
    // the search keeps icp_nn_grid_kernel's split between SGPRs and VGPRs.
    if (threadIdx.x < 12) s_m[threadIdx.x] = transforms[(size_t)job * 12 + threadIdx.x];
    if (threadIdx.x >= 64 && threadIdx.x < 67) s_geo[threadIdx.x - 64] = origin[(size_t)J.sc * 3 + (threadIdx.x - 64)];
    if (threadIdx.x == 128) { s_geo[3] = cell[J.sc]; s_geo[4] = r2; }
    __syncthreads();
    const double* m = s_m;
    GSSupport U;
    U.P = pts + (size_t)J.s0 * 3;
    U.ord = order + J.s0;
    U.sk = sorted_keys + J.s0;
    U.ns = J.ns;
    U.s0 = J.s0;
    U.geo = s_geo;
    U.sc = J.sc;
    const double h = cell[J.sc];
    U.grid = status[J.sc] == 0 && n_clouds <= GRID_MAX_CLOUDS && h > 0.0 && isfinite(h);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const int d = dims[(size_t)J.sc * 3 + a];
        U.dm[a] = d < 0 ? 0 : (d > GRID_DROPPED ? GRID_DROPPED : d);
    }

    double sum = 0.0;
    int cnt = 0;
    const int c1 = (int)min((long long)J.nq, (long long)c0 + GS_SLICE);
#pragma unroll 1
    for (int qi = c0 + wave; qi < c1; qi += GS_WAVES) {                  // ascending: the wave's part of the fixed fold; qi < c1 <= nq
        const double* Q = pts + ((size_t)J.q0 + qi) * 3;
        const double x = Q[0], y = Q[1], z = Q[2];
        double bd;
        int bj;
        gs_search(U, gs_uniform(sga_move_point(m, 0, x, y, z)), gs_uniform(sga_move_point(m, 1, x, y, z)), gs_uniform(sga_move_point(m, 2, x, y, z)), lane,
                  row_start[wave], row_excl[wave], bd, bj);
        if (bj != INT_MAX) {                                             // uniform over the wave: the butterfly left the same pair in every lane
            sum = __dadd_rn(sum, bd);
            cnt += 1;
        }
    }
    if (lane == 0) {
        red_sum[wave] = sum;
        red_cnt[wave] = cnt;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = red_sum[0];
        int n = red_cnt[0];
        for (int w = 1; w < GS_WAVES; ++w) {                             // the four waves in order
            s = __dadd_rn(s, red_sum[w]);
            n += red_cnt[w];
        }
        GSPartial* out = partials + (size_t)job * slices + c;
        out->sum = s;
        out->count = n;
    }
}

// One lane per job: the slices in ascending order.  A job that is not live, or whose ids or offsets are bad: 0 and 0.
__global__ __launch_bounds__(GS_THREADS) void geo_fold_kernel(const int* __restrict__ off, int n_clouds, int total_points,
                                                              const int* __restrict__ pairs, int n_pairs, int slices,
                                                              const int* __restrict__ live, const GSPartial* __restrict__ partials,
                                                              int* __restrict__ count, double* __restrict__ sum_d2) {
    const long long job = (long long)blockIdx.x * GS_THREADS + threadIdx.x;
    if (job >= n_pairs) return;
    const SgaCloudPair J = sga_cloud_pair(off, n_clouds, total_points, pairs, n_pairs, (int)job);
    double s = 0.0;
    long long n = 0;
    if (J.ok && !(live && live[job] == 0)) {
        const int my = (int)min((long long)slices, ((long long)J.nq + GS_SLICE - 1) / GS_SLICE);     // never past what was written
        for (int c = 0; c < my; ++c) {
            const GSPartial p = partials[(size_t)job * slices + c];
            s = __dadd_rn(s, p.sum);
            n += p.count;
        }
    }
    count[job] = (int)n;                                                 // n <= nq < 2^31
    sum_d2[job] = s;
}

long gs_slices(int max_queries) { return max_queries > 0 ? ((long)max_queries + GS_SLICE - 1) / GS_SLICE : 1; }

}  // namespace

static_assert(sizeof(GSPartial) == 16, "sga_score_transforms_workspace_bytes counts 16 bytes per (job, slice)");

extern "C" int sga_ransac_models(const double* corr, const int32_t* offsets, int n_jobs, int total_rows, const int32_t* samples,
                                 const int32_t* hyp_offsets, int total_hyp, int max_hyp, const int32_t* offsets_host,
                                 const int32_t* hyp_offsets_host, double* models, int32_t* valid, double* resid2, void* stream) {
    const char* who = "sga_ransac_models";
    SGA_CHECK_ARG(n_jobs >= 0 && total_rows >= 0 && total_hyp >= 0 && max_hyp >= 0,
                  "sga_ransac_models: negative count (n_jobs %d, total_rows %d, total_hyp %d, max_hyp %d)", n_jobs, total_rows, total_hyp, max_hyp);
    SGA_CHECK_ARG(max_hyp <= total_hyp, "sga_ransac_models: max_hyp %d exceeds total_hyp %d", max_hyp, total_hyp);
    SGA_CHECK_ARG(total_rows < INT_MAX / 6 && total_hyp < INT_MAX / 12, "sga_ransac_models: total_rows %d / total_hyp %d too large for int32 indexing",
                  total_rows, total_hyp);
    const SgaPrefix OFFSETS{"offsets", "decrease", "job", "total_rows", nullptr, nullptr};
    const SgaPrefix HYP_OFFSETS{"hyp_offsets", "decrease", "job", "total_hyp", "hypotheses", "max_hyp"};
    if (int rc = sga_check_prefix(who, OFFSETS, offsets_host, n_jobs, total_rows, SGA_ANY)) return rc;
    if (int rc = sga_check_prefix(who, HYP_OFFSETS, hyp_offsets_host, n_jobs, total_hyp, max_hyp)) return rc;
    if (n_jobs == 0 || total_hyp == 0 || max_hyp == 0) return SGA_OK;                        // nothing to write
    SGA_CHECK_ARG(offsets && hyp_offsets && samples && models && valid && resid2, "sga_ransac_models: null pointer");
    SGA_CHECK_ARG(corr || total_rows == 0, "sga_ransac_models: null corr with total_rows %d", total_rows);
    SGA_CHECK_ARG(sga_aligned(8, corr, models, resid2) && sga_aligned(4, offsets, samples, hyp_offsets, valid),
                  "sga_ransac_models: misaligned pointer (fp64 arrays need 8 bytes, int32 arrays 4)");
    const long g_tiles = ((long)max_hyp + GM_THREADS - 1) / GM_THREADS;
    if (int rc = sga_check_grid(who, g_tiles, 1, n_jobs, "split the job list")) return rc;
    hipLaunchKernelGGL(geo_models_kernel, dim3((unsigned)(g_tiles * n_jobs)), dim3(GM_THREADS), 0, static_cast<hipStream_t>(stream), corr, offsets,
                       total_rows, samples, hyp_offsets, total_hyp, (int)g_tiles, models, valid, resid2);
    SGA_CHECK_LAUNCH("sga_ransac_models");
    return SGA_OK;
}

extern "C" size_t sga_score_transforms_workspace_bytes(int n_pairs, int max_queries) {
    if (n_pairs <= 0 || max_queries < 0) return 0;
    return (size_t)n_pairs * (size_t)gs_slices(max_queries) * sizeof(GSPartial);
}

extern "C" int sga_score_transforms_grid(const double* pts, const int32_t* offsets, int n_clouds, int total_points, const int32_t* pairs,
                                         int n_pairs, int max_queries, const int32_t* offsets_host, const int32_t* pairs_host,
                                         const double* cell, const double* origin, const int32_t* dims, const int32_t* status,
                                         const int32_t* order, const int64_t* sorted_keys, const double* transforms, const int32_t* live,
                                         double r2, int32_t* count, double* sum_d2, void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "sga_score_transforms_grid";
    SGA_CHECK_ARG(n_clouds >= 0 && total_points >= 0 && n_pairs >= 0 && max_queries >= 0,
                  "sga_score_transforms_grid: negative count (n_clouds %d, total_points %d, n_pairs %d, max_queries %d)", n_clouds, total_points,
                  n_pairs, max_queries);
    SGA_CHECK_ARG(max_queries <= total_points, "sga_score_transforms_grid: max_queries %d exceeds total_points %d", max_queries, total_points);
    SGA_CHECK_ARG(r2 >= 0.0, "sga_score_transforms_grid: r2 must be >= 0 or +inf (got %g)", r2);
    const SgaPrefix OFFSETS{"offsets", "decrease", "cloud", "total_points", nullptr, nullptr};
    if (int rc = sga_check_prefix(who, OFFSETS, offsets_host, n_clouds, total_points, SGA_ANY)) return rc;
    if (int rc = sga_check_pairs(who, "cloud", pairs_host, n_pairs, offsets_host, n_clouds, max_queries, INT_MAX)) return rc;
    if (n_pairs == 0) return SGA_OK;                                                         // nothing to write
    const long slices = gs_slices(max_queries), f_tiles = ((long)n_pairs + GS_THREADS - 1) / GS_THREADS;
    // one workgroup of 256 threads per (job, slice): the count must fit an int, and the launch 2^32 threads
    SGA_CHECK_ARG(slices * n_pairs < (1L << 24), "sga_score_transforms_grid: %ld x %d workgroups of %d threads exceed the grid limit; split the job list",
                  slices, n_pairs, GS_THREADS);
    const size_t need = sga_score_transforms_workspace_bytes(n_pairs, max_queries);
    if (int rc = sga_check_workspace(who, need, workspace, workspace_bytes)) return rc;
    SGA_CHECK_ARG(offsets && pairs && transforms && count && sum_d2, "sga_score_transforms_grid: null pointer");
    SGA_CHECK_ARG(pts || total_points == 0, "sga_score_transforms_grid: null point array");
    SGA_CHECK_ARG(cell && origin && dims && status && (total_points == 0 || (order && sorted_keys)), "sga_score_transforms_grid: null grid array");
    SGA_CHECK_ARG(sga_aligned(8, pts, cell, origin, sorted_keys, transforms, sum_d2, workspace) &&
                      sga_aligned(4, offsets, pairs, dims, status, order, live, count),
                  "sga_score_transforms_grid: misaligned pointer (fp64 and int64 arrays and the workspace need 8 bytes, int32 arrays 4)");
    hipStream_t s = static_cast<hipStream_t>(stream);
    GSPartial* partials = static_cast<GSPartial*>(workspace);
    if (max_queries > 0)
        hipLaunchKernelGGL(geo_score_kernel, dim3((unsigned)(slices * n_pairs)), dim3(GS_THREADS), 0, s, pts, offsets, n_clouds, total_points, pairs,
                           n_pairs, (int)slices, cell, origin, dims, status, order, reinterpret_cast<const long long*>(sorted_keys), transforms, live,
                           r2, partials);
    hipLaunchKernelGGL(geo_fold_kernel, dim3((unsigned)f_tiles), dim3(GS_THREADS), 0, s, offsets, n_clouds, total_points, pairs, n_pairs, (int)slices,
                       live, static_cast<const GSPartial*>(partials), count, sum_d2);
    SGA_CHECK_LAUNCH("sga_score_transforms_grid");
    return SGA_OK;
}
