// Cross-cloud nearest neighbour through the SUPPORT cloud's cell grid: the search under ICP refinement and under the geometric score of a
// transform (Open3D's evaluate_registration).  The contract written in include/sgaligner_hip.h IS the definition; tests/icp_ref.py
// restates it in numpy.  For every input and every cell size the outputs are, as bit patterns, those of sga_nn_search (csrc/nnsearch.hip) on
// the moved queries, masked by d2 <= r2: the grid only decides how much of the support is looked at.
//
// Jobs are (query cloud, support cloud) pairs over clouds packed back to back (csrc/pair_jobs.h); the grid arrays are those of
// sga_voxel_keys / sga_voxel_cells (csrc/voxel.hip) for the same pts / offsets.  Every id, offset and index read from a device array is
// re-checked: a bad one makes the wave do nothing (or skip that candidate), never read or write out of bounds.  No atomics: the output is a
// pure function of the input.  Every fp64 operation is rounded on its own (explicit __d*_rn forms AND -ffp-contract=off for this file).
//
// THE WORK ITEM: one wave per query, four queries (consecutive rows of the job's query cloud) per workgroup -- vg_knn_kernel's, with a
// list of length one.  A list of one needs no LDS list and no merge: every lane keeps the best (d2, j) of the candidates it saw, by
// d2 < best || (d2 == best && j < best_j) -- candidates do not arrive in ascending j --, and a wave butterfly with the same comparison
// gives the wave's best; the lowest index among exactly equal minima wins whatever the order.  Several queries per wave would pay where
// the 27-cell block is nearly empty (cell ~ r on a surface: about 9 occupied cells, a handful of candidates), but each lane would then
// run its own row searches serially; that variant has not been measured and is not built.  LDS: the row table, 2 KiB per workgroup.
//
// The moved query: without transforms q' = q; with m = transforms[job] (row-major [R | t], m[0..8] = R, m[9..11] = t)
// x' = ((m0 x + m1 y) + m2 z) + m9, y' = ((m3 x + m4 y) + m5 z) + m10, z' = ((m6 x + m7 y) + m8 z) + m11, no fma.
//
// The walk is vg_knn_kernel's, written out here with a list of one; its helpers and the grid constants are wave_search.h's.  The query is NOT a point of the support cloud: its
// cell coordinate t_a = floor((q'_a - o_a) / h) may be negative, beyond dims_a, huge or infinite, so it is clamped IN FP64 to
// [0, dims_a - 1] before the conversion, and the block |k - c|inf <= R is centred at the clamped cell c.  Every (kx, ky) row of the block
// is one contiguous range of sorted positions: lane r finds row r's range by a lower and an upper bound on sorted_keys, the wave
// prefix-sums the lengths and walks the concatenated ranges 64 candidates at a time.  R = 1, 2, 4, 8, 16; the best found so far is kept
// from one R to the next (the blocks nest).  A block that covers the support's whole cell box ends the search: all that lies outside it
// are dropped points (a non-finite coordinate), whose d2 is NaN or +inf and never wins.  A query that is still undecided after R = 16, a
// query with a non-finite moved coordinate and every query against a support without a grid (status != 0) walks the whole support.
//
// WHY THE STOP RULE IS EXACT, ALSO FOR A CENTRE OUTSIDE THE BOX.  The argument at the head of voxel.hip never uses that the query lies
// in cell c; it uses c only to name the block.  After the block of radius R around c has been scanned, `best` is the best of the block.
// A kept support point p that is NOT in the block has, on some axis a, k_a <= c_a - R - 1 or k_a >= c_a + R + 1.  Only sides on which
// such cells exist count: 0 <= k_a <= dims_a - 1 for every kept point, so a side with c_a - R <= 0 (or c_a + R >= dims_a - 1) has no
// points beyond it and its gap is +inf.  Lower side: k_a = floor(t), t = fl(fl(p_a - o_a) / h) < k_a + 1, and the two roundings move t
// by at most 2^-52 relatively, so in real numbers p_a - o_a < (c_a - R) h (1 + 2^-51).  The face F = fl(o_a + fl((c_a - R) h)) differs
// from the real o_a + (c_a - R) h by at most 2^-52 (|o_a| + 2 (c_a + R + 1) h), and gap = fl(q'_a - F) from q'_a - F by at most
// 2^-53 (|q'_a| + |F|).  With scale_a = max(|o_a|, |q'_a|) + (c_a + R + 1) h all of these stay below 2^-49 scale_a, so the real
// q'_a - p_a exceeds g_a = gap - 2^-40 scale_a.  The upper side mirrors it with F = fl(o_a + fl((c_a + R + 1) h)), gap = fl(F - q'_a).
// None of this asks where q'_a lies: for a query beyond the box on that axis (c_a clamped to 0 or dims_a - 1) the side towards the box is
// a real face with a large positive gap, the side away from it has no cells and counts +inf; for a query between the faces the gaps are
// those of voxel.hip.  The rule requires every g_a > 0 (a NaN or a negative one -- a query so far out that scale_a overflows, or one that
// the rounding put on the wrong side of a face -- leaves the query undecided, which only costs a larger block).  With g = min_a g_a > 0
// every point outside the block has real |q' - p|^2 >= g^2; its computed d2 is at least the real one times (1 - 2^-50), the computed g g
// at most the real g^2 (1 + 2^-52).  Hence g g (1 - 2^-40) > bound, bound = min(r2, best d2 or +inf without one), implies computed
// d2 > bound for every such point: it fails d2 <= r2 or loses against `best` even on a tie.  Points INSIDE the block were scanned
// whatever cell the rounding put them in: membership is by the key, not by position.
#include "pair_jobs.h"
#include "rigid_solver.h"
#include "wave_search.h"

namespace {

constexpr int IG_THREADS = 256;
constexpr int IG_WAVES = 4;                        // queries per workgroup: one wave each
constexpr int IC_STATE_INTS = 8;                   // sga_icp's per-job state in int32 units: done, pad, then prev fitness / rmse as fp64

__global__ __launch_bounds__(IG_THREADS) void icp_nn_grid_kernel(const double* __restrict__ pts, const int* __restrict__ off, int n_clouds,
                                                                 int total_points, const int* __restrict__ pairs, int n_pairs,
                                                                 const int* __restrict__ out_off, int total_queries, int q_tiles,
                                                                 const double* __restrict__ cell, const double* __restrict__ origin,
                                                                 const int* __restrict__ dims, const int* __restrict__ status,
                                                                 const int* __restrict__ order, const long long* __restrict__ sorted_keys,
                                                                 const double* __restrict__ transforms, const int* __restrict__ done,
                                                                 double r2, int squared, double* __restrict__ out_d,
                                                                 int* __restrict__ out_i) {
    __shared__ int row_start[IG_WAVES][64], row_excl[IG_WAVES][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int job = blockIdx.x / q_tiles;
    const SgaPairJob J = sga_pair_job(off, n_clouds, total_points, pairs, n_pairs, out_off, total_queries, job);
    if (!J.ok) return;                                                   // no workgroup-wide barrier below: a wave may leave on its own
    if (done && done[job * IC_STATE_INTS]) return;                       // sga_icp: a finished job keeps the results of its last search
    const int qi = (blockIdx.x % q_tiles) * IG_WAVES + wave;
    if (qi >= J.nq) return;
    const int sc = pairs[2 * job + 1];                                   // in [0, n_clouds): sga_pair_job checked it
    if (sc < 0 || sc >= n_clouds) return;

    const double* Q = pts + ((size_t)J.q0 + qi) * 3;
    double qx = Q[0], qy = Q[1], qz = Q[2];
    if (transforms) {
        const double* m = transforms + (size_t)job * 12;
        const double x = qx, y = qy, z = qz;
        qx = sga_move_point(m, 0, x, y, z);
        qy = sga_move_point(m, 1, x, y, z);
        qz = sga_move_point(m, 2, x, y, z);
    }
    const double* P = pts + (size_t)J.s0 * 3;
    const int* ord = order + J.s0;
    const long long* sk = sorted_keys + J.s0;
    int* rs = row_start[wave];
    int* rx = row_excl[wave];

    const double h = cell[sc];
    int kc[3], dm[3];
    bool use_grid = status[sc] == 0 && n_clouds <= GRID_MAX_CLOUDS && h > 0.0 && isfinite(h) && isfinite(qx) && isfinite(qy) && isfinite(qz);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const int d = dims[(size_t)sc * 3 + a];
        dm[a] = d < 0 ? 0 : (d > GRID_DROPPED ? GRID_DROPPED : d);
        const double qa = a == 0 ? qx : (a == 1 ? qy : qz);
        double t = floor(__ddiv_rn(__dsub_rn(qa, origin[(size_t)sc * 3 + a]), h));
        use_grid = use_grid && dm[a] > 0 && t == t;                      // no kept point, or a NaN: the whole walk
        t = fmin(fmax(t, 0.0), (double)(dm[a] > 0 ? dm[a] - 1 : 0));     // clamped in fp64: t may be -inf, +inf or beyond any int
        kc[a] = t == t ? (int)t : 0;
    }
    const long long cloud_bits = (long long)sc << 48;

    double bd = INFINITY;
    int bj = INT_MAX;
    bool decided = false;
    if (use_grid) {
#pragma unroll 1
        for (int R = 1; R <= GRID_MAX_R && !decided; R *= 2) {
            const int x0 = max(kc[0] - R, 0), y0 = max(kc[1] - R, 0), z0 = max(kc[2] - R, 0);
            const int x1 = min(kc[0] + R, dm[0] - 1), y1 = min(kc[1] + R, dm[1] - 1), z1 = min(kc[2] + R, dm[2] - 1);
            const int ny = y1 - y0 + 1, rows = (x1 - x0 + 1) * ny;       // at most 33 x 33
#pragma unroll 1
            for (int rb = 0; rb < rows; rb += 64) {
                const int r = rb + lane;
                int start = 0, len = 0;
                if (r < rows) {
                    const long long rowkey = cloud_bits | ((long long)(x0 + r / ny) << 32) | ((long long)(y0 + r % ny) << 16);
                    start = sga_lower_bound(sk, J.ns, rowkey | (long long)z0);
                    len = sga_lower_bound(sk, J.ns, (rowkey | (long long)z1) + 1) - start;
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
                    const bool tin = t >= 0 && t < J.ns;
                    const int i = tin ? ord[t] : J.s0;
                    const bool jin = tin && i >= J.s0 && i - J.s0 < J.ns;
                    const int j = jin ? i - J.s0 : 0;
                    const double d2 = sga_point_d2(qx, qy, qz, P + (size_t)j * 3);          // total_len > 0: the support has a row 0
                    sga_nn_offer(r2, d2, j, inb && jin, bd, bj);
                }
            }
            sga_wave_best(bd, bj);
            if (x0 == 0 && y0 == 0 && z0 == 0 && x1 == dm[0] - 1 && y1 == dm[1] - 1 && z1 == dm[2] - 1) { decided = true; break; }   // the whole box
            // the stop rule: see the head of this file
            const double bound = fmin(r2, bd);
            double g = INFINITY;
            bool ok = true;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const double o = origin[(size_t)sc * 3 + a], qa = a == 0 ? qx : (a == 1 ? qy : qz);
                const double scale = __dadd_rn(fmax(fabs(o), fabs(qa)), __dmul_rn((double)(kc[a] + R + 1), h));
                double gap = INFINITY;
                if (kc[a] - R > 0) gap = __dsub_rn(qa, __dadd_rn(o, __dmul_rn((double)(kc[a] - R), h)));
                if (kc[a] + R < dm[a] - 1) {
                    const double up = __dsub_rn(__dadd_rn(o, __dmul_rn((double)(kc[a] + R + 1), h)), qa);
                    ok = ok && up == up && gap == gap;
                    gap = fmin(gap, up);
                }
                const double ga = __dsub_rn(gap, __dmul_rn(GRID_EPS, scale));
                ok = ok && ga > 0.0;                                     // a NaN is not > 0
                g = fmin(g, ga);
            }
            if (ok && g > 0.0 && __dmul_rn(__dmul_rn(g, g), 1.0 - GRID_EPS) > bound) decided = true;
        }
    }
    if (!decided) {                                                      // the whole support in original order, as nn_kernel looks at it
        bd = INFINITY;
        bj = INT_MAX;
        for (int j = lane; j < J.ns; j += 64) sga_nn_offer(r2, sga_point_d2(qx, qy, qz, P + (size_t)j * 3), j, true, bd, bj);
        sga_wave_best(bd, bj);
    }
    if (lane == 0) {
        out_d[(size_t)J.oo + qi] = squared ? bd : __dsqrt_rn(bd);
        out_i[(size_t)J.oo + qi] = bj == INT_MAX ? -1 : bj;
    }
}

// ---- ICP: accumulate and step -------------------------------------------------------------------------------------------------------------
// sga_icp enqueues max_iters + 1 rounds of { icp_nn_grid_kernel with the job's current transform, icp_accum_kernel, icp_step_kernel } on
// one stream and never synchronises: a finished job raises its `done` flag in the workspace and the workgroups of later rounds leave at
// once, so its out_idx / out_d2 stay those of its final transform.  Open3D's loop: evaluate; repeat { update, evaluate, stop when both
// changes are small }.
//
// icp_accum_kernel: a slice is IC_SLICE query rows counted from the job's first row; one workgroup per (job, slice).  Over the rows with a
// partner (out_idx >= 0, re-checked against the support's length): slot 0 the count, slot 1 sum d2, then with a = x' - pivot (x' recomputed by
// the search's own expression) and b = s - pivot, method 0: sum a (3), sum b (3), sum a b^T (9) -- rigid_from_moments' layout --; method 1,
// with n the partner's normal, r = (a - b) . n and J = [a x n, n]: the 21 upper entries of sum J J^T (row by row), the 6 of sum J r, sum r r.
// The fold is fixed: every lane its IC_RPL rows in ascending order, a wave butterfly, the four waves in order; icp_step_kernel adds the
// slices in ascending order.  No atomics: two calls give the same bits, and a job in a batch gives the bits of the same job alone.
constexpr int IC_THREADS = 256;
constexpr int IC_RPL = 4;                          // query rows per lane
constexpr int IC_SLICE = IC_THREADS * IC_RPL;      // query rows per slice
constexpr int IC_ACC = 32;                         // slots of a partial: 17 used by method 0, 30 by method 1

struct ICState { int done, pad; double prev_fitness, prev_rmse, pad1; };
static_assert(sizeof(ICState) == IC_STATE_INTS * 4, "icp_nn_grid_kernel reads the done flag by this stride");

template <int METHOD>
__global__ __launch_bounds__(IC_THREADS) void icp_accum_kernel(const double* __restrict__ pts, const double* __restrict__ normals,
                                                               const int* __restrict__ off, int n_clouds, int total_points,
                                                               const int* __restrict__ pairs, int n_pairs, const int* __restrict__ out_off,
                                                               int total_queries, int slices, const double* __restrict__ transforms,
                                                               const double* __restrict__ pivot, const ICState* __restrict__ state,
                                                               const double* __restrict__ out_d2, const int* __restrict__ out_idx,
                                                               double* __restrict__ partials) {
    constexpr int N = METHOD == 0 ? 17 : 30;
    __shared__ double red[IC_THREADS / 64][IC_ACC];
    const int tid = threadIdx.x, job = blockIdx.x / slices, c = blockIdx.x % slices;
    const SgaPairJob J = sga_pair_job(off, n_clouds, total_points, pairs, n_pairs, out_off, total_queries, job);
    if (!J.ok || state[job].done) return;
    const int c0 = c * IC_SLICE;                                         // c < slices <= ceil(max_queries / IC_SLICE): no overflow
    if (c0 >= J.nq) return;
    double m[12], piv[3], acc[N];
#pragma unroll
    for (int a = 0; a < 12; ++a) m[a] = transforms[(size_t)job * 12 + a];
#pragma unroll
    for (int a = 0; a < 3; ++a) piv[a] = pivot[(size_t)job * 3 + a];
#pragma unroll
    for (int a = 0; a < N; ++a) acc[a] = 0.0;
#pragma unroll
    for (int k = 0; k < IC_RPL; ++k) {
        const int i = c0 + k * IC_THREADS + tid;
        if (i >= J.nq) continue;
        const int j = out_idx[(size_t)J.oo + i];
        if (j < 0 || j >= J.ns) continue;
        const double* Q = pts + ((size_t)J.q0 + i) * 3;
        const double* S = pts + ((size_t)J.s0 + j) * 3;
        const double x = Q[0], y = Q[1], z = Q[2];
        double a[3], b[3];
#pragma unroll
        for (int e = 0; e < 3; ++e) {
            a[e] = sga_move_point(m, e, x, y, z) - piv[e];
            b[e] = S[e] - piv[e];
        }
        acc[0] += 1.0;
        acc[1] += out_d2[(size_t)J.oo + i];
        if (METHOD == 0) {
#pragma unroll
            for (int e = 0; e < 3; ++e) { acc[2 + e] += a[e]; acc[5 + e] += b[e]; }
#pragma unroll
            for (int e = 0; e < 3; ++e)
#pragma unroll
                for (int f = 0; f < 3; ++f) acc[8 + 3 * e + f] += a[e] * b[f];
        } else {
            const double* Nn = normals + ((size_t)J.s0 + j) * 3;
            const double nx = Nn[0], ny = Nn[1], nz = Nn[2];
            const double r = ((a[0] - b[0]) * nx + (a[1] - b[1]) * ny) + (a[2] - b[2]) * nz;
            const double Jv[6] = {a[1] * nz - a[2] * ny, a[2] * nx - a[0] * nz, a[0] * ny - a[1] * nx, nx, ny, nz};
            int s = 2;
#pragma unroll
            for (int e = 0; e < 6; ++e)
#pragma unroll
                for (int f = e; f < 6; ++f) acc[s++] += Jv[e] * Jv[f];
#pragma unroll
            for (int e = 0; e < 6; ++e) acc[23 + e] += Jv[e] * r;
            acc[29] += r * r;
        }
    }
#pragma unroll
    for (int a = 0; a < N; ++a) acc[a] = wave_sum_d(acc[a]);
    if ((tid & 63) == 0) {
#pragma unroll
        for (int a = 0; a < N; ++a) red[tid >> 6][a] = acc[a];
    }
    __syncthreads();
    if (tid < N) {
        double s = red[0][tid];
        for (int w = 1; w < IC_THREADS / 64; ++w) s += red[w][tid];
        partials[((size_t)job * slices + c) * IC_ACC + tid] = s;
    }
}

// Method 1's update from the folded sums S (slots 2 .. 28): (sum J J^T) x = -sum J r by Cholesky without pivoting, every index a
// compile-time constant; a pivot that is <= 0 or not finite: false.  Then R_U = Rz(x2) Ry(x1) Rx(x0), t_U = (x3, x4, x5) + pivot - R_U pivot.
__device__ inline bool ic_plane_update(const double* S, const double* piv, double* out) {
    double L[6][6], x[6];
    {
        int s = 2;
#pragma unroll
        for (int e = 0; e < 6; ++e)
#pragma unroll
            for (int f = e; f < 6; ++f) L[f][e] = S[s++];                 // the lower triangle
    }
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        double d = L[j][j];
#pragma unroll
        for (int k = 0; k < j; ++k) d -= L[j][k] * L[j][k];
        if (!(d > 0.0) || !isfinite(d)) return false;
        const double ljj = sqrt(d);
        L[j][j] = ljj;
#pragma unroll
        for (int i = j + 1; i < 6; ++i) {
            double v = L[i][j];
#pragma unroll
            for (int k = 0; k < j; ++k) v -= L[i][k] * L[j][k];
            L[i][j] = v / ljj;
        }
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) {                                        // L y = -b
        double v = -S[23 + i];
#pragma unroll
        for (int k = 0; k < i; ++k) v -= L[i][k] * x[k];
        x[i] = v / L[i][i];
    }
#pragma unroll
    for (int i = 5; i >= 0; --i) {                                       // L^T x = y
        double v = x[i];
#pragma unroll
        for (int k = i + 1; k < 6; ++k) v -= L[k][i] * x[k];
        x[i] = v / L[i][i];
    }
    const double ca = cos(x[0]), sa = sin(x[0]), cb = cos(x[1]), sb = sin(x[1]), cg = cos(x[2]), sg = sin(x[2]);
    const double R[9] = {cg * cb, cg * sb * sa - sg * ca, cg * sb * ca + sg * sa,
                         sg * cb, sg * sb * sa + cg * ca, sg * sb * ca - cg * sa,
                         -sb, cb * sa, cb * ca};
    bool fin = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        out[9 + a] = (x[3 + a] + piv[a]) - ((R[3 * a] * piv[0] + R[3 * a + 1] * piv[1]) + R[3 * a + 2] * piv[2]);
        fin = fin && isfinite(out[9 + a]);
    }
#pragma unroll
    for (int a = 0; a < 9; ++a) { out[a] = R[a]; fin = fin && isfinite(R[a]); }
    return fin;
}

// Evaluation k of max_iters: fold the slices, write fitness / rmse to the trace, decide, update the transform (T <- U T).
__global__ __launch_bounds__(64) void icp_step_kernel(const int* __restrict__ off, int n_clouds, int total_points, const int* __restrict__ pairs,
                                                      int n_pairs, const int* __restrict__ out_off, int total_queries, int slices,
                                                      const double* __restrict__ partials, const double* __restrict__ pivot, int method, int k,
                                                      int max_iters, double rel_fitness, double rel_rmse, ICState* __restrict__ state,
                                                      double* __restrict__ transform, double* __restrict__ fitness, double* __restrict__ rmse,
                                                      int* __restrict__ iters, int* __restrict__ status, double* __restrict__ trace) {
    __shared__ double S[IC_ACC];
    const int tid = threadIdx.x, job = blockIdx.x;
    const SgaPairJob J = sga_pair_job(off, n_clouds, total_points, pairs, n_pairs, out_off, total_queries, job);
    ICState* st = state + job;
    if (!J.ok) {                                                         // nothing of such a job was searched: status 3, once
        if (tid == 0 && k == 0) { st->done = 1; status[job] = 3; iters[job] = 0; fitness[job] = 0.0; rmse[job] = 0.0; }
        if (k == 0)
            for (int e = tid; e < 2 * (max_iters + 1); e += 64) trace[(size_t)job * 2 * (max_iters + 1) + e] = NAN;
        return;
    }
    if (st->done) return;                                                // uniform over the workgroup
    if (k == 0)
        for (int e = tid; e < 2 * (max_iters + 1); e += 64) trace[(size_t)job * 2 * (max_iters + 1) + e] = NAN;
    if (tid < IC_ACC) {
        const int my = (int)min((long long)slices, ((long long)J.nq + IC_SLICE - 1) / IC_SLICE);
        double s = 0.0;
        for (int c = 0; c < my; ++c) s += partials[((size_t)job * slices + c) * IC_ACC + tid];      // ascending: a fixed order
        S[tid] = s;
    }
    __syncthreads();                                                     // also orders the NaN fill before the two trace entries below
    if (tid != 0) return;
    const double cnt = S[0];
    const double fit = J.nq > 0 ? cnt / (double)J.nq : 0.0, rm = cnt > 0.0 ? sqrt(S[1] / cnt) : 0.0;
    double* tr = trace + ((size_t)job * (max_iters + 1) + k) * 2;
    tr[0] = fit;
    tr[1] = rm;
    fitness[job] = fit;
    rmse[job] = rm;
    iters[job] = k;
    int stt = 0;
    bool done = k == max_iters || (k >= 1 && fabs(fit - st->prev_fitness) < rel_fitness && fabs(rm - st->prev_rmse) < rel_rmse);
    st->prev_fitness = fit;
    st->prev_rmse = rm;
    if (!done) {
        double U[12], piv[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) piv[a] = pivot[(size_t)job * 3 + a];
        bool ok;
        if (cnt < (method == 0 ? 3.0 : 6.0)) {
            ok = false;
            stt = 1;
        } else {
            ok = method == 0 ? rigid_from_moments(cnt, S + 2, piv, piv, U) : ic_plane_update(S, piv, U);
            if (!ok) stt = 2;
        }
        if (ok) {
            double* T = transform + (size_t)job * 12;
            double N[12];
#pragma unroll
            for (int a = 0; a < 3; ++a) {
#pragma unroll
                for (int b = 0; b < 3; ++b) N[3 * a + b] = (U[3 * a] * T[b] + U[3 * a + 1] * T[3 + b]) + U[3 * a + 2] * T[6 + b];
                N[9 + a] = ((U[3 * a] * T[9] + U[3 * a + 1] * T[10]) + U[3 * a + 2] * T[11]) + U[9 + a];
            }
            bool fin = true;
#pragma unroll
            for (int a = 0; a < 12; ++a) fin = fin && isfinite(N[a]);
            if (fin) {
#pragma unroll
                for (int a = 0; a < 12; ++a) T[a] = N[a];
            } else {
                stt = 2;
            }
        }
        done = stt != 0;
    }
    status[job] = stt;
    if (done) st->done = 1;
}

// sga_icp's workspace: the per-job state, then the partials.
size_t ic_state_bytes(int n_pairs) { return (size_t)n_pairs * sizeof(ICState); }
long ic_slices(int max_queries) { return max_queries > 0 ? ((long)max_queries + IC_SLICE - 1) / IC_SLICE : 1; }

}  // namespace

extern "C" size_t sga_icp_workspace_bytes(int n_pairs, int max_queries) {
    if (n_pairs <= 0 || max_queries < 0) return 0;
    return ic_state_bytes(n_pairs) + (size_t)n_pairs * (size_t)ic_slices(max_queries) * IC_ACC * sizeof(double);
}

extern "C" int sga_icp(const double* pts, const int32_t* offsets, int n_clouds, int total_points, const int32_t* pairs, int n_pairs,
                       const int32_t* out_offsets, int total_queries, int max_queries, const int32_t* offsets_host, const int32_t* pairs_host,
                       const double* cell, const double* origin, const int32_t* dims, const int32_t* grid_status, const int32_t* order,
                       const int64_t* sorted_keys, double r2, int method, const double* normals, const double* pivot, int max_iters,
                       double rel_fitness, double rel_rmse, double* transform, double* fitness, double* inlier_rmse, int32_t* iters,
                       int32_t* status, double* trace, int32_t* out_idx, double* out_d2, void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "sga_icp";
    SGA_CHECK_ARG(n_clouds >= 0 && total_points >= 0 && n_pairs >= 0 && total_queries >= 0 && max_queries >= 0,
                  "sga_icp: negative count (n_clouds %d, total_points %d, n_pairs %d, total_queries %d, max_queries %d)", n_clouds, total_points,
                  n_pairs, total_queries, max_queries);
    SGA_CHECK_ARG(max_queries <= total_queries, "sga_icp: max_queries %d exceeds total_queries %d", max_queries, total_queries);
    SGA_CHECK_ARG(r2 >= 0.0, "sga_icp: r2 must be >= 0 or +inf (got %g)", r2);
    SGA_CHECK_ARG(method == 0 || method == 1, "sga_icp: method must be 0 (point-to-point) or 1 (point-to-plane) (got %d)", method);
    SGA_CHECK_ARG(max_iters >= 0 && max_iters <= 100000, "sga_icp: max_iters must be in [0, 100000] (got %d)", max_iters);
    SGA_CHECK_ARG(rel_fitness == rel_fitness && rel_rmse == rel_rmse, "sga_icp: rel_fitness / rel_rmse must not be NaN");
    SGA_CHECK_ARG(method == 0 || normals || total_points == 0, "sga_icp: method 1 (point-to-plane) needs the support normals");
    const SgaPrefix OFFSETS{"offsets", "decrease", "cloud", "total_points", nullptr, nullptr};
    if (int rc = sga_check_prefix(who, OFFSETS, offsets_host, n_clouds, total_points, SGA_ANY)) return rc;
    if (int rc = sga_check_pairs(who, "cloud", pairs_host, n_pairs, offsets_host, n_clouds, max_queries, INT_MAX)) return rc;
    if (n_pairs == 0) return SGA_OK;
    const size_t need = sga_icp_workspace_bytes(n_pairs, max_queries);
    if (int rc = sga_check_workspace(who, need, workspace, workspace_bytes)) return rc;
    SGA_CHECK_ARG(offsets && pairs && out_offsets && pivot && transform && fitness && inlier_rmse && iters && status && trace, "sga_icp: null pointer");
    SGA_CHECK_ARG((out_idx && out_d2) || total_queries == 0, "sga_icp: null pointer");
    SGA_CHECK_ARG(pts || total_points == 0, "sga_icp: null point array");
    SGA_CHECK_ARG(cell && origin && dims && grid_status && (total_points == 0 || (order && sorted_keys)), "sga_icp: null grid array");
    SGA_CHECK_ARG(sga_aligned(8, pts, normals, pivot, cell, origin, sorted_keys, transform, fitness, inlier_rmse, trace, out_d2, workspace) &&
                      sga_aligned(4, offsets, pairs, out_offsets, dims, grid_status, order, iters, status, out_idx),
                  "sga_icp: misaligned pointer (fp64 and int64 arrays and the workspace need 8 bytes, int32 arrays 4)");
    const long q_tiles = ((long)max_queries + IG_WAVES - 1) / IG_WAVES, slices = ic_slices(max_queries);
    if (int rc = sga_check_grid(who, q_tiles > 0 ? q_tiles : 1, 1, n_pairs, "split the job list")) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (int rc = sga_zero(who, workspace, need, s)) return rc;                    // done flags and partials start at zero
    ICState* state = static_cast<ICState*>(workspace);
    double* partials = reinterpret_cast<double*>(static_cast<char*>(workspace) + ic_state_bytes(n_pairs));
    const long long* sk64 = reinterpret_cast<const long long*>(sorted_keys);
    for (int k = 0; k <= max_iters; ++k) {
        if (max_queries > 0) {
            hipLaunchKernelGGL(icp_nn_grid_kernel, dim3((unsigned)(q_tiles * n_pairs)), dim3(IG_THREADS), 0, s, pts, offsets, n_clouds, total_points,
                               pairs, n_pairs, out_offsets, total_queries, (int)q_tiles, cell, origin, dims, grid_status, order, sk64,
                               static_cast<const double*>(transform), reinterpret_cast<const int*>(state), r2, 1, out_d2, out_idx);
            if (method == 0)
                hipLaunchKernelGGL(icp_accum_kernel<0>, dim3((unsigned)(slices * n_pairs)), dim3(IC_THREADS), 0, s, pts, normals, offsets, n_clouds,
                                   total_points, pairs, n_pairs, out_offsets, total_queries, (int)slices, static_cast<const double*>(transform), pivot,
                                   static_cast<const ICState*>(state), static_cast<const double*>(out_d2), static_cast<const int*>(out_idx), partials);
            else
                hipLaunchKernelGGL(icp_accum_kernel<1>, dim3((unsigned)(slices * n_pairs)), dim3(IC_THREADS), 0, s, pts, normals, offsets, n_clouds,
                                   total_points, pairs, n_pairs, out_offsets, total_queries, (int)slices, static_cast<const double*>(transform), pivot,
                                   static_cast<const ICState*>(state), static_cast<const double*>(out_d2), static_cast<const int*>(out_idx), partials);
        }
        hipLaunchKernelGGL(icp_step_kernel, dim3((unsigned)n_pairs), dim3(64), 0, s, offsets, n_clouds, total_points, pairs, n_pairs, out_offsets,
                           total_queries, (int)slices, static_cast<const double*>(partials), pivot, method, k, max_iters, rel_fitness, rel_rmse, state,
                           transform, fitness, inlier_rmse, iters, status, trace);
    }
    SGA_CHECK_LAUNCH("sga_icp");
    return SGA_OK;
}

extern "C" int sga_nn_search_grid(const double* pts, const int32_t* offsets, int n_clouds, int total_points, const int32_t* pairs, int n_pairs,
                                  const int32_t* out_offsets, int total_queries, int max_queries, const int32_t* offsets_host,
                                  const int32_t* pairs_host, const double* cell, const double* origin, const int32_t* dims, const int32_t* status,
                                  const int32_t* order, const int64_t* sorted_keys, const double* transforms, double r2, int squared,
                                  double* out_dist, int32_t* out_idx, void* stream) {
    const char* who = "sga_nn_search_grid";
    SGA_CHECK_ARG(n_clouds >= 0 && total_points >= 0 && n_pairs >= 0 && total_queries >= 0 && max_queries >= 0,
                  "sga_nn_search_grid: negative count (n_clouds %d, total_points %d, n_pairs %d, total_queries %d, max_queries %d)", n_clouds,
                  total_points, n_pairs, total_queries, max_queries);
    SGA_CHECK_ARG(max_queries <= total_queries, "sga_nn_search_grid: max_queries %d exceeds total_queries %d", max_queries, total_queries);
    SGA_CHECK_ARG(r2 >= 0.0, "sga_nn_search_grid: r2 must be >= 0 or +inf (got %g)", r2);
    const SgaPrefix OFFSETS{"offsets", "decrease", "cloud", "total_points", nullptr, nullptr};
    if (int rc = sga_check_prefix(who, OFFSETS, offsets_host, n_clouds, total_points, SGA_ANY)) return rc;
    if (int rc = sga_check_pairs(who, "cloud", pairs_host, n_pairs, offsets_host, n_clouds, max_queries, INT_MAX)) return rc;
    if (n_pairs == 0 || total_queries == 0 || max_queries == 0) return SGA_OK;               // nothing to write
    SGA_CHECK_ARG(offsets && pairs && out_offsets && out_dist && out_idx, "sga_nn_search_grid: null pointer");
    SGA_CHECK_ARG(pts || total_points == 0, "sga_nn_search_grid: null point array");
    SGA_CHECK_ARG(cell && origin && dims && status && (total_points == 0 || (order && sorted_keys)), "sga_nn_search_grid: null grid array");
    SGA_CHECK_ARG(sga_aligned(8, pts, out_dist, cell, origin, sorted_keys, transforms) && sga_aligned(4, offsets, pairs, out_offsets, out_idx, dims, status, order),
                  "sga_nn_search_grid: misaligned pointer (fp64 and int64 arrays need 8 bytes, int32 arrays 4)");
    const long q_tiles = ((long)max_queries + IG_WAVES - 1) / IG_WAVES;
    if (int rc = sga_check_grid(who, q_tiles, 1, n_pairs, "split the job list")) return rc;
    hipLaunchKernelGGL(icp_nn_grid_kernel, dim3((unsigned)(q_tiles * n_pairs)), dim3(IG_THREADS), 0, static_cast<hipStream_t>(stream), pts, offsets,
                       n_clouds, total_points, pairs, n_pairs, out_offsets, total_queries, (int)q_tiles, cell, origin, dims, status, order,
                       reinterpret_cast<const long long*>(sorted_keys), transforms, static_cast<const int*>(nullptr), r2, squared, out_dist,
                       out_idx);
    SGA_CHECK_LAUNCH("sga_nn_search_grid");
    return SGA_OK;
}
