// A uniform cell grid over every cloud of a packed batch, and its two consumers: voxel down-sampling (utils/open3d.py:68-76) and
// grid-accelerated neighbour lists that are bit-equal to sga_knn_lists (csrc/fpfh.hip).  The contract written in include/sgaligner_hip.h IS
// the definition; tests/voxel_ref.py restates the grid and the means in numpy, tests/fpfh_ref.lists_ref is the yardstick of the lists.
//
// Clouds are packed back to back (csrc/packed.h).  Every kernel re-checks each offset, index and count it reads: a bad one makes it do
// nothing (or skip that entry), never read or write out of bounds.  No atomics anywhere: every output is a pure function of the input.
// Every fp64 operation is rounded on its own (explicit __d*_rn forms AND -ffp-contract=off for this file).
//
// The grid: vx_bounds_kernel (one workgroup per cloud: min / max of the kept points, origin = min - h / 2, dims, status),
// vx_keys_kernel (one lane per point: key = cloud << 48 | kx << 32 | ky << 16 | kz), then -- the 64-bit sort is borrowed: `order` is an
// INPUT -- vx_verify_kernel (order is the stable argsort of the keys: every entry inside its cloud, (key, index) strictly increasing),
// vx_heads_kernel / vx_scan_totals_kernel / vx_scan_kernel (head flags, their exclusive prefix sum: a block scan in LDS plus one
// workgroup over the block totals) and vx_finish_kernel (voxel ids, run heads, per-cloud prefix, status).
//
// vx_means_kernel: one lane per voxel, the sequential sum of the run in sorted order (= ascending original index) divided by its length.
//
// vg_knn_kernel: one wave per query, queries taken in SORTED order (the four queries of a workgroup are neighbours), results written at
// the original row.  For the block of cells |k - c|inf <= R around the query's cell c, every (kx, ky) row of the block is one contiguous
// range of sorted positions (kz is the lowest key field): lane r finds row r's range with a lower and an upper bound on sorted_keys, the
// wave prefix-sums the lengths and walks the concatenated ranges 64 candidates at a time (a lane finds its candidate's row by a binary
// search over the 64 prefix entries in LDS), with the d2 expression of knn_kernel and its ballot / stage / rank-sort merge (kl_rank_sort of
// wave_search.h; vg_merge / vg_offer are this file's list state around it).  Candidates do not arrive in ascending j, so admission against a full list is
// lexicographic: d2 < tau || (d2 == tau && j < tau_j).  R = 1, 2, 4, 8, 16, each from an empty list; a query that is still undecided, one whose
// block would cover the cloud's whole cell box, a dropped query and every query of a cloud without a grid (status != 0) streams its whole
// cloud in original order instead, as knn_kernel does.  Either way the list is the first max_nn of {j : d2 <= r2} by (d2, j): the grid
// only decides how much of the cloud is looked at.
//
// WHY THE STOP RULE IS EXACT.  After the block of radius R has been scanned, the list holds the best of the block.  A point p of the cloud
// that is NOT in the block has, on some axis a, a cell coordinate k_a < c_a - R or k_a > c_a + R.  Only sides on which such cells exist
// count: k_a >= 0 always, and k_a <= dims_a - 1 (k is monotone in p, dims comes from the cloud's max with the same three operations), so a
// side on which the block reaches the box has no points beyond it and its gap is +inf.  Take k_a <= c_a - R - 1 (the other side mirrors
// it).  k_a = floor(t), t = fl(fl(p_a - o_a) / h) <= k_a + 1 - ulp, and the two roundings move t by at most 2^-52 relatively, so in real
// numbers p_a - o_a < (k_a + 1) h (1 + 2^-51) <= (c_a - R) h + 2^-51 (|c_a| + R + 1) h.  The kernel's face F = fl(o_a + fl((c_a - R) h)) differs
// from the real o_a + (c_a - R) h by at most 2^-52 (|o_a| + 2 (|c_a| + R + 1) h), and gap = fl(q_a - F) from q_a - F by at most 2^-53 (|q_a| +
// |F|).  With scale_a = max(|o_a|, |q_a|) + (|c_a| + R + 1) h all of these together stay below 2^-49 scale_a, so the real distance
// q_a - p_a exceeds gap_a - 2^-40 scale_a =: g_a with a factor 2^9 to spare, and |q - p|^2 >= g^2 for g = min_a g_a > 0.  The computed
// d2 = fl(fl(dx dx + dy dy) + dz dz) of such a point is at least the real |q - p|^2 (1 - 2^-50) (each of the three subtractions, three
// products and two sums errs by 2^-53 relatively and all terms are non-negative), and the computed g g is at most the real g^2 (1 + 2^-52).
// Hence g g (1 - 2^-40) > bound implies computed d2 > bound for every point outside the block, where bound = min(r2, tau if the list is
// full else +inf): such a point fails d2 <= r2 or loses against the full list even on a tie (d2 > tau strictly), so scanning it would not
// change the list.  Points INSIDE the block were scanned whatever cell the rounding put them in: membership is by the key, not by position.
#include "pair_jobs.h"
#include "wave_search.h"

namespace {

constexpr int VX_THREADS = 256;
constexpr int VX_ITEMS = 4;                        // sorted positions per lane in the scan kernels
constexpr int VX_BLOCK = VX_THREADS * VX_ITEMS;    // sorted positions per workgroup in the scan kernels
constexpr long long VX_CELL_MASK = 0xFFFFFFFFFFFFll;

constexpr int KL_THREADS = 256;
constexpr int KL_WAVES = 4;                        // queries per workgroup: one wave each
constexpr int KL_MAX_NN = 128;                     // longest list
constexpr int KL_STAGE = 64;                       // staged candidates per wave: one full ballot
constexpr int KL_SLOTS = KL_MAX_NN + KL_STAGE;     // entries a merge sorts, three per lane at most
__device__ __forceinline__ long long vx_dropped_key(int c) { return ((long long)c << 48) | VX_CELL_MASK; }
__device__ __forceinline__ bool vx_is_dropped(long long key) { return (key & VX_CELL_MASK) == VX_CELL_MASK; }

// ---- bounds, origin, dims ----------------------------------------------------------------------------------------------------------------
// One workgroup per cloud.  With `box` ([n_clouds, 6]: min xyz | max xyz of the kept points, +inf | -inf without one) it writes the bounds
// and, with `edge`, the cell edge at which a cell holds about per_cell points (sga_cloud_bounds; the rule is in the header) and nothing
// else; otherwise origin, dims and status from `cell`.
__global__ __launch_bounds__(VX_THREADS) void vx_bounds_kernel(const double* __restrict__ pts, const int* __restrict__ off, int n_clouds,
                                                               int total_points, const double* __restrict__ cell, double* __restrict__ origin,
                                                               int* __restrict__ dims, int* __restrict__ status, double* __restrict__ box,
                                                               double per_cell, double* __restrict__ edge) {
    __shared__ double smn[3][VX_THREADS / 64], smx[3][VX_THREADS / 64];
    const int c = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (c >= n_clouds) return;
    const SgaCloud C = sga_cloud(off, total_points, c);
    double mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int j = tid; j < C.n; j += VX_THREADS) {                       // C.n == 0 on a bad offset
        const double* p = pts + ((size_t)C.o0 + j) * 3;
        const double x = p[0], y = p[1], z = p[2];
        if (isfinite(x) && isfinite(y) && isfinite(z)) {
            mn[0] = fmin(mn[0], x); mn[1] = fmin(mn[1], y); mn[2] = fmin(mn[2], z);
            mx[0] = fmax(mx[0], x); mx[1] = fmax(mx[1], y); mx[2] = fmax(mx[2], z);
        }
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            mn[a] = fmin(mn[a], __shfl_xor(mn[a], o, 64));
            mx[a] = fmax(mx[a], __shfl_xor(mx[a], o, 64));
        }
        if (lane == 0) { smn[a][wave] = mn[a]; smx[a][wave] = mx[a]; }
    }
    __syncthreads();
    if (tid != 0) return;
    if (box) {
        double e[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            double lo = smn[a][0], hi = smx[a][0];
#pragma unroll
            for (int w = 1; w < VX_THREADS / 64; ++w) { lo = fmin(lo, smn[a][w]); hi = fmax(hi, smx[a][w]); }
            box[(size_t)c * 6 + a] = lo;
            box[(size_t)c * 6 + 3 + a] = hi;
            e[a] = lo <= hi ? hi - lo : 0.0;
        }
        if (edge) {                                                     // a speed choice, never part of a result: plain arithmetic
            const double e1 = fmax(e[0], fmax(e[1], e[2])), e3 = fmin(e[0], fmin(e[1], e[2])), e2 = ((e[0] + e[1]) + e[2]) - e1 - e3;
            const double share = per_cell / (double)(C.n > 0 ? C.n : 1);
            double h = sqrt(e1 * e2 * share);
            if (!(h > 0.0)) h = e1 * share;
            h = fmax(h, e1 / 60000.0);
            edge[c] = (h > 0.0 && isfinite(h)) ? h : 1.0;
        }
        return;
    }
    const double h = cell[c];
    const bool h_ok = C.ok && h > 0.0 && isfinite(h);
    int st = (h_ok && n_clouds <= GRID_MAX_CLOUDS) ? 0 : 2;
    double o[3] = {0.0, 0.0, 0.0};
    int d[3] = {0, 0, 0};
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        double lo = smn[a][0], hi = smx[a][0];
#pragma unroll
        for (int w = 1; w < VX_THREADS / 64; ++w) { lo = fmin(lo, smn[a][w]); hi = fmax(hi, smx[a][w]); }
        if (h_ok && lo <= hi) {                                         // the cloud has a kept point
            o[a] = __dsub_rn(lo, __dmul_rn(0.5, h));
            const double kd = floor(__ddiv_rn(__dsub_rn(hi, o[a]), h));
            if (kd >= 0.0 && kd < (double)GRID_DROPPED) d[a] = (int)kd + 1; else st = 2;
        }
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        origin[(size_t)c * 3 + a] = o[a];
        dims[(size_t)c * 3 + a] = st == 0 ? d[a] : 0;
    }
    status[c] = st;
}

// ---- keys --------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(VX_THREADS) void vx_keys_kernel(const double* __restrict__ pts, const int* __restrict__ off, int n_clouds,
                                                             int total_points, const double* __restrict__ cell, const double* __restrict__ origin,
                                                             const int* __restrict__ status, long long* __restrict__ keys) {
    const long long gi = (long long)blockIdx.x * VX_THREADS + threadIdx.x;
    if (gi >= total_points) return;
    const int i = (int)gi;
    const SgaCloud C = sga_cloud_of_point(off, n_clouds, total_points, i);
    const int cf = n_clouds <= GRID_MAX_CLOUDS ? C.c : 0;
    long long key = vx_dropped_key(cf);
    if (C.ok && status[C.c] == 0) {
        const double h = cell[C.c];
        int k[3];
        bool kept = true;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const double p = pts[(size_t)i * 3 + a];
            const double kd = floor(__ddiv_rn(__dsub_rn(p, origin[(size_t)C.c * 3 + a]), h));
            kept = kept && isfinite(p) && kd >= 0.0 && kd < (double)GRID_DROPPED;
            k[a] = kept ? (int)kd : GRID_DROPPED;
        }
        if (kept) key = ((long long)cf << 48) | ((long long)k[0] << 32) | ((long long)k[1] << 16) | (long long)k[2];
    }
    keys[i] = key;
}

// ---- the borrowed sort, verified ---------------------------------------------------------------------------------------------------------
// Position t of cloud c: order[t] lies in the cloud, and (key, index) at t - 1 is strictly below (key, index) at t.  All positions of a
// cloud passing proves a stable permutation: strictly increasing pairs are distinct, an index has one key, so the n entries are n distinct
// indices of the cloud in (key, index) order.  A failing position flags its cloud (every writer stores the same 1).
__global__ __launch_bounds__(VX_THREADS) void vx_verify_kernel(const int* __restrict__ off, int n_clouds, int total_points,
                                                               const long long* __restrict__ keys, const int* __restrict__ order,
                                                               long long* __restrict__ sorted_keys, int* __restrict__ bad) {
    const long long gt = (long long)blockIdx.x * VX_THREADS + threadIdx.x;
    if (gt >= total_points) return;
    const int t = (int)gt;
    const SgaCloud C = sga_cloud_of_point(off, n_clouds, total_points, t);
    if (!C.ok) { sorted_keys[t] = vx_dropped_key(0); return; }
    const int i = order[t];
    if (i < C.o0 || i - C.o0 >= C.n) {
        bad[C.c] = 1;
        sorted_keys[t] = vx_dropped_key(C.c);
        return;
    }
    const long long k = keys[i];
    sorted_keys[t] = k;
    if (t > C.o0) {
        const int ip = order[t - 1];
        if (ip >= C.o0 && ip - C.o0 < C.n) {                            // an index outside is flagged by position t - 1
            const long long kp = keys[ip];
            if (!(kp < k || (kp == k && ip < i))) bad[C.c] = 1;
        }
    }
}

// ---- heads and their exclusive prefix sum ------------------------------------------------------------------------------------------------
__device__ __forceinline__ int vx_block_sum(int v, int* __restrict__ sw) {      // sum over the workgroup, to every lane
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int incl = wave_incl_scan(v, lane);
    if (lane == 63) sw[wave] = incl;
    __syncthreads();
    int tot = 0;
#pragma unroll
    for (int w = 0; w < VX_THREADS / 64; ++w) tot += sw[w];
    return tot;
}

// exclusive prefix of v over the workgroup in thread order; `tot` gets the workgroup's sum
__device__ __forceinline__ int vx_block_excl(int v, int* __restrict__ sw, int& tot) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int incl = wave_incl_scan(v, lane);
    if (lane == 63) sw[wave] = incl;
    __syncthreads();
    int before = 0;
    tot = 0;
#pragma unroll
    for (int w = 0; w < VX_THREADS / 64; ++w) {
        before += w < wave ? sw[w] : 0;
        tot += sw[w];
    }
    return before + incl - v;
}

// flag[t] = 1 when sorted position t starts a voxel: a kept point of a cloud whose grid and order stand, first of its cloud or of its key.
__global__ __launch_bounds__(VX_THREADS) void vx_heads_kernel(const int* __restrict__ off, int n_clouds, int total_points,
                                                              const long long* __restrict__ sorted_keys, const int* __restrict__ status,
                                                              const int* __restrict__ bad, int* __restrict__ scan, int* __restrict__ block_tot) {
    __shared__ int sw[VX_THREADS / 64];
    const long long base = (long long)blockIdx.x * VX_BLOCK + (long long)threadIdx.x * VX_ITEMS;
    int mine = 0;
#pragma unroll
    for (int e = 0; e < VX_ITEMS; ++e) {
        const long long gt = base + e;
        if (gt >= total_points) break;
        const int t = (int)gt;
        const SgaCloud C = sga_cloud_of_point(off, n_clouds, total_points, t);
        int head = 0;
        if (C.ok && status[C.c] == 0 && bad[C.c] == 0) {
            const long long k = sorted_keys[t];
            head = !vx_is_dropped(k) && (t == C.o0 || sorted_keys[t - 1] != k);
        }
        scan[t] = head;
        mine += head;
    }
    const int tot = vx_block_sum(mine, sw);
    if (threadIdx.x == 0) block_tot[blockIdx.x] = tot;
}

// One workgroup: block_tot[0 .. n_blocks) -> its exclusive prefix in place, block_tot[n_blocks] = the grand total.
__global__ __launch_bounds__(VX_THREADS) void vx_scan_totals_kernel(int* __restrict__ block_tot, int n_blocks) {
    __shared__ int sw[VX_THREADS / 64];
    int carry = 0;
    for (int b0 = 0; b0 < n_blocks; b0 += VX_THREADS) {
        const int b = b0 + threadIdx.x;
        const int v = b < n_blocks ? block_tot[b] : 0;
        int tot;
        const int ex = vx_block_excl(v, sw, tot);
        if (b < n_blocks) block_tot[b] = carry + ex;
        carry += tot;
        __syncthreads();                                                // sw is reused by the next round
    }
    if (threadIdx.x == 0) block_tot[n_blocks] = carry;
}

// scan[t]: head flag -> the number of heads at positions < t; scan[total_points] = the number of voxels of the call.
__global__ __launch_bounds__(VX_THREADS) void vx_scan_kernel(int total_points, int n_blocks, const int* __restrict__ block_tot, int* __restrict__ scan) {
    __shared__ int sw[VX_THREADS / 64];
    const long long base = (long long)blockIdx.x * VX_BLOCK + (long long)threadIdx.x * VX_ITEMS;
    int f[VX_ITEMS], mine = 0;
#pragma unroll
    for (int e = 0; e < VX_ITEMS; ++e) {
        f[e] = base + e < total_points ? scan[base + e] : 0;
        mine += f[e];
    }
    int tot;
    int run = block_tot[blockIdx.x] + vx_block_excl(mine, sw, tot);
#pragma unroll
    for (int e = 0; e < VX_ITEMS; ++e) {
        if (base + e < total_points) scan[base + e] = run;
        run += f[e];
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) scan[total_points] = block_tot[n_blocks];
}

// Voxel ids, run heads, the per-cloud prefix and the final status.  Lane t serves sorted position t and, for t <= n_clouds, cloud t.
__global__ __launch_bounds__(VX_THREADS) void vx_finish_kernel(const int* __restrict__ off, int n_clouds, int total_points,
                                                               const int* __restrict__ order, const long long* __restrict__ sorted_keys,
                                                               const int* __restrict__ scan, const int* __restrict__ bad,
                                                               int* __restrict__ voxel_of_point, int* __restrict__ voxel_offsets,
                                                               int* __restrict__ voxel_first, int* __restrict__ status) {
    const long long gt = (long long)blockIdx.x * VX_THREADS + threadIdx.x;
    if (gt < total_points) {
        const int t = (int)gt;
        const SgaCloud C = sga_cloud_of_point(off, n_clouds, total_points, t);
        const bool valid = C.ok && status[C.c] == 0 && bad[C.c] == 0;      // status[c] may already read 3 here: bad[c] says the same
        if (!valid) {
            voxel_of_point[t] = -1;                                        // by position: the order of such a cloud is not trusted
        } else {
            const int i = order[t];
            if (i >= C.o0 && i - C.o0 < C.n) {                             // verified; re-checked all the same
                const long long k = sorted_keys[t];
                const bool head = !vx_is_dropped(k) && (t == C.o0 || sorted_keys[t - 1] != k);
                const int id = head ? scan[t] : scan[t] - 1;               // global voxel id of t's run
                if (vx_is_dropped(k)) {
                    voxel_of_point[i] = -1;
                } else {
                    voxel_of_point[i] = id - scan[C.o0];
                    if (head && id >= 0 && id < total_points) voxel_first[id] = t;
                }
            }
        }
    }
    if (gt <= n_clouds) {
        const int c = (int)gt;
        const int o = off[c];
        voxel_offsets[c] = scan[o < 0 ? 0 : (o > total_points ? total_points : o)];
        if (c == n_clouds) {
            const int nv = scan[total_points];
            if (nv >= 0 && nv <= total_points) voxel_first[nv] = total_points;
        } else if (status[c] == 0 && bad[c] != 0) {
            status[c] = 3;
        }
    }
}

// ---- voxel means -------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(VX_THREADS) void vx_means_kernel(const double* __restrict__ pts, const double* __restrict__ normals,
                                                              const int* __restrict__ off, int n_clouds, int total_points,
                                                              const int* __restrict__ order, const long long* __restrict__ sorted_keys,
                                                              const int* __restrict__ voxel_offsets, const int* __restrict__ voxel_first,
                                                              const int* __restrict__ status, double* __restrict__ out_pts,
                                                              double* __restrict__ out_normals, int* __restrict__ out_count) {
    const long long gv = (long long)blockIdx.x * VX_THREADS + threadIdx.x;
    const int n_vox = voxel_offsets[n_clouds];
    if (gv >= n_vox || gv >= total_points) return;
    const int g = (int)gv;
    int lo = 0, hi = n_clouds - 1;                                          // the LAST cloud whose first voxel id is <= g
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (voxel_offsets[mid] <= g) lo = mid; else hi = mid - 1;
    }
    const SgaCloud C = sga_cloud(off, total_points, lo);
    if (!C.ok || status[lo] != 0 || voxel_offsets[lo] > g || voxel_offsets[lo + 1] <= g) return;
    const int s = voxel_first[g];
    if (s < C.o0 || s - C.o0 >= C.n) return;
    const long long key = sorted_keys[s];
    double sx = 0.0, sy = 0.0, sz = 0.0, nx = 0.0, ny = 0.0, nz = 0.0;
    int m = 0;
    for (int t = s; t < C.o0 + C.n && sorted_keys[t] == key; ++t) {          // the run ends where the key changes
        const int i = order[t];
        if (i < C.o0 || i - C.o0 >= C.n) continue;
        sx = __dadd_rn(sx, pts[(size_t)i * 3]);
        sy = __dadd_rn(sy, pts[(size_t)i * 3 + 1]);
        sz = __dadd_rn(sz, pts[(size_t)i * 3 + 2]);
        if (normals) {
            nx = __dadd_rn(nx, normals[(size_t)i * 3]);
            ny = __dadd_rn(ny, normals[(size_t)i * 3 + 1]);
            nz = __dadd_rn(nz, normals[(size_t)i * 3 + 2]);
        }
        ++m;
    }
    const double dm = (double)m;
    out_pts[(size_t)g * 3] = __ddiv_rn(sx, dm);
    out_pts[(size_t)g * 3 + 1] = __ddiv_rn(sy, dm);
    out_pts[(size_t)g * 3 + 2] = __ddiv_rn(sz, dm);
    if (normals && out_normals) {
        out_normals[(size_t)g * 3] = __ddiv_rn(nx, dm);
        out_normals[(size_t)g * 3 + 1] = __ddiv_rn(ny, dm);
        out_normals[(size_t)g * 3 + 2] = __ddiv_rn(nz, dm);
    }
    out_count[g] = m;
}

// ---- grid neighbour lists ----------------------------------------------------------------------------------------------------------------
// The wave's list: L sorted entries, S staged behind them; full: tau / tau_j are the max_nn-th best (d2, j).
struct VgList { int L, S; double tau; int tau_j; bool full; };

__device__ __forceinline__ void vg_reset(VgList& q) { q.L = 0; q.S = 0; q.tau = INFINITY; q.tau_j = INT_MAX; q.full = false; }

__device__ __forceinline__ void vg_merge(double* __restrict__ wd, int* __restrict__ wi, int lane, int max_nn, VgList& q) {
    const int E = q.L + q.S;
    sga_wave_sync();
    if (E <= 64) kl_rank_sort<1, 1>(wd, wi, lane, q.L, E, max_nn);
    else if (E <= 128) kl_rank_sort<2, 1>(wd, wi, lane, q.L, E, max_nn);
    else kl_rank_sort<3, 1>(wd, wi, lane, q.L, E, max_nn);
    q.L = min(E, max_nn);
    q.S = 0;
    if (E >= max_nn) { q.full = true; q.tau = wd[max_nn - 1]; q.tau_j = wi[max_nn - 1]; }
}

// Lane's candidate (d2, j), live when inb: admitted iff d2 <= r2 and, against a full list, (d2, j) < (tau, tau_j).  A stale tau only
// admits too much; the merge drops it again.
__device__ __forceinline__ void vg_offer(double* __restrict__ wd, int* __restrict__ wi, int lane, int max_nn, double r2, double d2, int j,
                                         bool inb, VgList& q) {
    bool adm = inb && d2 <= r2 && (!q.full || sga_d2j_less(d2, j, q.tau, q.tau_j));      // a NaN fails d2 <= r2
    unsigned long long bal = __ballot(adm);
    if (bal == 0ull) return;
    int c = __popcll(bal);
    if (q.S + c > KL_STAGE) {
        vg_merge(wd, wi, lane, max_nn, q);
        adm = adm && (!q.full || sga_d2j_less(d2, j, q.tau, q.tau_j));
        bal = __ballot(adm);
        c = __popcll(bal);
    }
    if (adm) {
        const int slot = q.L + q.S + __popcll(bal & ((1ull << lane) - 1ull));       // < max_nn + 64
        wd[slot] = d2;
        wi[slot] = j;
    }
    q.S += c;
}

// Five waves per SIMD = five workgroups per CU (95 VGPRs; knn_kernel holds 7 by its LDS): a sixth costs 11 spilled registers.
__global__ __launch_bounds__(KL_THREADS) __attribute__((amdgpu_waves_per_eu(5))) void vg_knn_kernel(const double* __restrict__ pts, const int* __restrict__ off, int n_clouds,
                                                            int total_points, const double* __restrict__ cell, const double* __restrict__ origin,
                                                            const int* __restrict__ dims, const int* __restrict__ status,
                                                            const int* __restrict__ order, const long long* __restrict__ sorted_keys, double r2,
                                                            int max_nn, int* __restrict__ out_count, int* __restrict__ out_idx,
                                                            double* __restrict__ out_d2) {
    __shared__ double list_d[KL_WAVES][KL_SLOTS];
    __shared__ int list_i[KL_WAVES][KL_SLOTS];
    __shared__ int row_start[KL_WAVES][64], row_excl[KL_WAVES][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long gp = (long long)blockIdx.x * KL_WAVES + wave;
    if (gp >= total_points) return;                                      // no workgroup-wide barrier below: a wave may leave on its own
    const int pos = (int)gp;
    const SgaCloud C = sga_cloud_of_point(off, n_clouds, total_points, pos);
    if (!C.ok) return;
    const bool has_grid = status[C.c] == 0;
    int qi = pos;                                                        // without a grid: the query at its own row
    long long key = vx_dropped_key(0);
    if (has_grid) {
        qi = order[pos];
        if (qi < C.o0 || qi - C.o0 >= C.n) return;
        key = sorted_keys[pos];
    }
    const double* P = pts + (size_t)C.o0 * 3;
    const int* ord = order + C.o0;
    const long long* sk = sorted_keys + C.o0;
    const double qx = pts[(size_t)qi * 3], qy = pts[(size_t)qi * 3 + 1], qz = pts[(size_t)qi * 3 + 2];
    double* wd = list_d[wave];
    int* wi = list_i[wave];
    int* rs = row_start[wave];
    int* rx = row_excl[wave];
    VgList q;

    const int kc[3] = {(int)((key >> 32) & 0xFFFF), (int)((key >> 16) & 0xFFFF), (int)(key & 0xFFFF)};
    int dm[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const int d = dims[(size_t)C.c * 3 + a];
        dm[a] = d < 0 ? 0 : (d > GRID_DROPPED ? GRID_DROPPED : d);
    }
    const bool use_grid = has_grid && !vx_is_dropped(key) && kc[0] < dm[0] && kc[1] < dm[1] && kc[2] < dm[2] && cell[C.c] > 0.0;
    const long long cloud_bits = key & ~VX_CELL_MASK;
    // One pass per block radius R = 1, 2, 4, 8, 16, each from an empty list; R = 0 is the pass over the whole cloud in original order (as
    // knn_kernel walks it, dropped points included): a single "row" [0, n) read without `order`.  It is the last pass whenever it runs.
#pragma unroll 1
    for (int R = use_grid ? 1 : 0;; R *= 2) {
        if (R > GRID_MAX_R) R = 0;
        int x0 = 0, y0 = 0, z0 = 0, z1 = 0, ny = 1, rows = 1;
        if (R > 0) {
            const int x1 = min(kc[0] + R, dm[0] - 1), y1 = min(kc[1] + R, dm[1] - 1);
            x0 = max(kc[0] - R, 0); y0 = max(kc[1] - R, 0); z0 = max(kc[2] - R, 0);
            z1 = min(kc[2] + R, dm[2] - 1);
            if (x0 == 0 && y0 == 0 && z0 == 0 && x1 == dm[0] - 1 && y1 == dm[1] - 1 && z1 == dm[2] - 1) R = 0;      // the whole box
            ny = y1 - y0 + 1;
            rows = (x1 - x0 + 1) * ny;
        }
        const bool whole = R == 0;
        if (whole) rows = 1;
        vg_reset(q);
#pragma unroll 1
        for (int rb = 0; rb < rows; rb += 64) {
            const int r = rb + lane;
            int start = 0, len = 0;
            if (whole) {
                len = lane == 0 ? C.n : 0;
            } else if (r < rows) {
                const long long rowkey = cloud_bits | ((long long)(x0 + r / ny) << 32) | ((long long)(y0 + r % ny) << 16);
                start = sga_lower_bound(sk, C.n, rowkey | (long long)z0);
                len = sga_lower_bound(sk, C.n, (rowkey | (long long)z1) + 1) - start;
                if (len < 0) len = 0;
            }
            const int incl = wave_incl_scan(len, lane);
            const int total_len = __shfl(incl, 63, 64);
            sga_wave_sync();                                              // the previous batch's table has been read by every lane
            rs[lane] = start;
            rx[lane] = incl - len;
            sga_wave_sync();
#pragma unroll 1
            for (int u0 = 0; u0 < total_len; u0 += 64) {
                const bool inb = u0 + lane < total_len;
                const int u = inb ? u0 + lane : total_len - 1;
                int lo = 0;                                              // the LAST row whose exclusive prefix is <= u: rows of length 0 are passed over
#pragma unroll
                for (int step = 32; step > 0; step >>= 1)
                    if (rx[lo + step] <= u) lo += step;                  // lo + step <= 63
                const int t = rs[lo] + (u - rx[lo]);
                const bool tin = t >= 0 && t < C.n;
                const int i = !tin ? C.o0 : (whole ? C.o0 + t : ord[t]);
                const bool jin = tin && i >= C.o0 && i - C.o0 < C.n;
                const int j = jin ? i - C.o0 : 0;
                const double d2 = sga_point_d2(qx, qy, qz, P + (size_t)j * 3);
                vg_offer(wd, wi, lane, max_nn, r2, d2, j, inb && jin, q);
            }
        }
        if (q.S > 0) vg_merge(wd, wi, lane, max_nn, q);
        if (whole) break;
        // the stop rule: see the head of this file
        const double bound = fmin(r2, q.full ? q.tau : INFINITY);
        const double h = cell[C.c];
        double g = INFINITY;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const double o = origin[(size_t)C.c * 3 + a], qa = a == 0 ? qx : (a == 1 ? qy : qz);
            const double scale = __dadd_rn(fmax(fabs(o), fabs(qa)), __dmul_rn((double)(kc[a] + R + 1), h));
            double gap = INFINITY;
            if (kc[a] - R > 0) gap = __dsub_rn(qa, __dadd_rn(o, __dmul_rn((double)(kc[a] - R), h)));
            if (kc[a] + R < dm[a] - 1) gap = fmin(gap, __dsub_rn(__dadd_rn(o, __dmul_rn((double)(kc[a] + R + 1), h)), qa));
            g = fmin(g, __dsub_rn(gap, __dmul_rn(GRID_EPS, scale)));
        }
        if (g > 0.0 && __dmul_rn(__dmul_rn(g, g), 1.0 - GRID_EPS) > bound) break;
    }
    sga_wave_sync();
    const size_t row = (size_t)qi * max_nn;
    for (int e = lane; e < max_nn; e += 64) {
        out_idx[row + e] = e < q.L ? wi[e] : -1;
        out_d2[row + e] = e < q.L ? wd[e] : INFINITY;
    }
    if (lane == 0) out_count[qi] = q.L;
}

// ---- host --------------------------------------------------------------------------------------------------------------------------------
size_t vx_round8(size_t b) { return (b + 7) / 8 * 8; }
int vx_blocks(int total_points) { return (int)(((long long)total_points + VX_BLOCK - 1) / VX_BLOCK); }

// What the entries check alike: counts and the offsets' host copy.
int vx_check(const char* who, const void* offsets, int n_clouds, int total_points, const int32_t* offsets_host) {
    SGA_CHECK_ARG(n_clouds >= 0 && total_points >= 0, "%s: negative count (n_clouds %d, total_points %d)", who, n_clouds, total_points);
    SGA_CHECK_ARG(total_points < INT_MAX - VX_BLOCK, "%s: total_points %d is too large", who, total_points);
    const SgaPrefix OFFSETS{"offsets", "decrease", "cloud", "total_points", nullptr, nullptr};
    if (int rc = sga_check_prefix(who, OFFSETS, offsets_host, n_clouds, total_points, SGA_ANY)) return rc;
    SGA_CHECK_ARG(offsets || n_clouds == 0 || total_points == 0, "%s: null offsets", who);
    SGA_CHECK_ARG(sga_aligned(4, offsets), "%s: misaligned offsets (int32 arrays need 4 bytes)", who);
    return SGA_OK;
}

}  // namespace

extern "C" size_t sga_voxel_workspace_bytes(int n_clouds, int total_points) {
    if (n_clouds < 0 || total_points < 0) return 0;
    return vx_round8(4 * ((size_t)n_clouds + 1)) + vx_round8(4 * ((size_t)vx_blocks(total_points) + 1)) + vx_round8(4 * ((size_t)total_points + 1));
}

extern "C" int sga_cloud_bounds(const double* pts, const int32_t* offsets, int n_clouds, int total_points, const int32_t* offsets_host, double* box,
                                double per_cell, double* edge, void* stream) {
    if (int rc = vx_check("sga_cloud_bounds", offsets, n_clouds, total_points, offsets_host)) return rc;
    if (n_clouds == 0) return SGA_OK;
    SGA_CHECK_ARG(box && (pts || total_points == 0), "sga_cloud_bounds: null pointer");
    SGA_CHECK_ARG(sga_aligned(8, pts, box, edge), "sga_cloud_bounds: misaligned pointer (fp64 arrays need 8 bytes)");
    SGA_CHECK_ARG(!edge || (per_cell > 0.0 && per_cell <= 1e9), "sga_cloud_bounds: per_cell must be > 0 (got %g)", per_cell);
    if (int rc = sga_check_grid("sga_cloud_bounds", n_clouds, 1, 1, "split the cloud list")) return rc;
    hipLaunchKernelGGL(vx_bounds_kernel, dim3((unsigned)n_clouds), dim3(VX_THREADS), 0, static_cast<hipStream_t>(stream), pts, offsets, n_clouds,
                       total_points, static_cast<const double*>(nullptr), static_cast<double*>(nullptr), static_cast<int*>(nullptr),
                       static_cast<int*>(nullptr), box, per_cell, edge);
    SGA_CHECK_LAUNCH("sga_cloud_bounds");
    return SGA_OK;
}

extern "C" int sga_voxel_keys(const double* pts, const int32_t* offsets, int n_clouds, int total_points, const int32_t* offsets_host,
                              const double* cell, const double* cell_host, double* origin, int32_t* dims, int64_t* keys, int32_t* status,
                              void* stream) {
    if (int rc = vx_check("sga_voxel_keys", offsets, n_clouds, total_points, offsets_host)) return rc;
    if (cell_host)
        for (int c = 0; c < n_clouds; ++c)
            SGA_CHECK_ARG(cell_host[c] > 0.0 && cell_host[c] <= 1.7e308, "sga_voxel_keys: cell must be > 0 and finite (cloud %d: %g)", c, cell_host[c]);
    if (n_clouds == 0) return SGA_OK;
    SGA_CHECK_ARG(cell && origin && dims && status && (pts || total_points == 0) && (keys || total_points == 0), "sga_voxel_keys: null pointer");
    SGA_CHECK_ARG(sga_aligned(8, pts, cell, origin, keys) && sga_aligned(4, dims, status),
                  "sga_voxel_keys: misaligned pointer (fp64 and int64 arrays need 8 bytes, int32 arrays 4)");
    if (int rc = sga_check_grid("sga_voxel_keys", n_clouds, 1, 1, "split the cloud list")) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(vx_bounds_kernel, dim3((unsigned)n_clouds), dim3(VX_THREADS), 0, s, pts, offsets, n_clouds, total_points, cell, origin, dims,
                       status, static_cast<double*>(nullptr), 0.0, static_cast<double*>(nullptr));
    SGA_CHECK_LAUNCH("sga_voxel_keys");
    if (total_points == 0) return SGA_OK;
    const long grid = ((long)total_points + VX_THREADS - 1) / VX_THREADS;
    hipLaunchKernelGGL(vx_keys_kernel, dim3((unsigned)grid), dim3(VX_THREADS), 0, s, pts, offsets, n_clouds, total_points, cell, origin, status,
                       reinterpret_cast<long long*>(keys));
    SGA_CHECK_LAUNCH("sga_voxel_keys");
    return SGA_OK;
}

extern "C" int sga_voxel_cells(const int32_t* offsets, int n_clouds, int total_points, const int32_t* offsets_host, const int64_t* keys,
                               const int32_t* order, int64_t* sorted_keys, int32_t* voxel_of_point, int32_t* voxel_offsets,
                               int32_t* voxel_first, int32_t* status, void* workspace, size_t workspace_bytes, void* stream) {
    if (int rc = vx_check("sga_voxel_cells", offsets, n_clouds, total_points, offsets_host)) return rc;
    if (n_clouds == 0) return SGA_OK;
    if (int rc = sga_check_workspace("sga_voxel_cells", sga_voxel_workspace_bytes(n_clouds, total_points), workspace, workspace_bytes)) return rc;
    SGA_CHECK_ARG(voxel_offsets && voxel_first && status && (total_points == 0 || (keys && order && sorted_keys && voxel_of_point)),
                  "sga_voxel_cells: null pointer");
    SGA_CHECK_ARG(sga_aligned(8, keys, sorted_keys, workspace) && sga_aligned(4, order, voxel_of_point, voxel_offsets, voxel_first, status),
                  "sga_voxel_cells: misaligned pointer (int64 arrays and the workspace need 8 bytes, int32 arrays 4)");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int n_blocks = vx_blocks(total_points);
    char* w = static_cast<char*>(workspace);
    int* bad = reinterpret_cast<int*>(w);
    int* block_tot = reinterpret_cast<int*>(w + vx_round8(4 * ((size_t)n_clouds + 1)));
    int* scan = reinterpret_cast<int*>(w + vx_round8(4 * ((size_t)n_clouds + 1)) + vx_round8(4 * ((size_t)n_blocks + 1)));
    // bad flags, block totals and scan[total_points] start at zero (with no point there is no scan kernel to write the last)
    if (int rc = sga_zero("sga_voxel_cells", workspace, sga_voxel_workspace_bytes(n_clouds, total_points), s)) return rc;
    const long long* k64 = reinterpret_cast<const long long*>(keys);
    long long* sk64 = reinterpret_cast<long long*>(sorted_keys);
    if (total_points > 0) {
        const long grid = ((long)total_points + VX_THREADS - 1) / VX_THREADS;
        hipLaunchKernelGGL(vx_verify_kernel, dim3((unsigned)grid), dim3(VX_THREADS), 0, s, offsets, n_clouds, total_points, k64, order, sk64, bad);
        hipLaunchKernelGGL(vx_heads_kernel, dim3((unsigned)n_blocks), dim3(VX_THREADS), 0, s, offsets, n_clouds, total_points, sk64, status, bad, scan,
                           block_tot);
        hipLaunchKernelGGL(vx_scan_totals_kernel, dim3(1), dim3(VX_THREADS), 0, s, block_tot, n_blocks);
        hipLaunchKernelGGL(vx_scan_kernel, dim3((unsigned)n_blocks), dim3(VX_THREADS), 0, s, total_points, n_blocks, block_tot, scan);
    }
    const long lanes = (long)(total_points > n_clouds + 1 ? total_points : n_clouds + 1);
    hipLaunchKernelGGL(vx_finish_kernel, dim3((unsigned)((lanes + VX_THREADS - 1) / VX_THREADS)), dim3(VX_THREADS), 0, s, offsets, n_clouds,
                       total_points, order, sk64, scan, bad, voxel_of_point, voxel_offsets, voxel_first, status);
    SGA_CHECK_LAUNCH("sga_voxel_cells");
    return SGA_OK;
}

extern "C" int sga_voxel_downsample(const double* pts, const double* normals, const int32_t* offsets, int n_clouds, int total_points,
                                    const int32_t* offsets_host, const int32_t* order, const int64_t* sorted_keys, const int32_t* voxel_offsets,
                                    const int32_t* voxel_first, const int32_t* status, double* out_pts, double* out_normals, int32_t* out_count,
                                    void* stream) {
    if (int rc = vx_check("sga_voxel_downsample", offsets, n_clouds, total_points, offsets_host)) return rc;
    if (n_clouds == 0 || total_points == 0) return SGA_OK;
    SGA_CHECK_ARG(pts && order && sorted_keys && voxel_offsets && voxel_first && status && out_pts && out_count, "sga_voxel_downsample: null pointer");
    SGA_CHECK_ARG(!normals == !out_normals, "sga_voxel_downsample: normals and out_normals go together");
    SGA_CHECK_ARG(sga_aligned(8, pts, normals, sorted_keys, out_pts, out_normals) && sga_aligned(4, order, voxel_offsets, voxel_first, status, out_count),
                  "sga_voxel_downsample: misaligned pointer (fp64 and int64 arrays need 8 bytes, int32 arrays 4)");
    const long grid = ((long)total_points + VX_THREADS - 1) / VX_THREADS;
    hipLaunchKernelGGL(vx_means_kernel, dim3((unsigned)grid), dim3(VX_THREADS), 0, static_cast<hipStream_t>(stream), pts, normals, offsets, n_clouds,
                       total_points, order, reinterpret_cast<const long long*>(sorted_keys), voxel_offsets, voxel_first, status, out_pts,
                       out_normals, out_count);
    SGA_CHECK_LAUNCH("sga_voxel_downsample");
    return SGA_OK;
}

extern "C" int sga_knn_lists_grid(const double* pts, const int32_t* offsets, int n_clouds, int total_points, const int32_t* offsets_host,
                                  const double* cell, const double* origin, const int32_t* dims, const int32_t* status, const int32_t* order,
                                  const int64_t* sorted_keys, double r2, int max_nn, int32_t* count, int32_t* idx, double* d2, void* stream) {
    if (int rc = vx_check("sga_knn_lists_grid", offsets, n_clouds, total_points, offsets_host)) return rc;
    SGA_CHECK_ARG(max_nn >= 1 && max_nn <= KL_MAX_NN, "sga_knn_lists_grid: max_nn must be in [1, %d] (got %d)", KL_MAX_NN, max_nn);
    SGA_CHECK_ARG((long long)total_points * max_nn < (1LL << 31), "sga_knn_lists_grid: total_points x max_nn must stay below 2^31 (%d x %d)",
                  total_points, max_nn);
    SGA_CHECK_ARG(r2 >= 0.0, "sga_knn_lists_grid: r2 must be >= 0 or +inf (got %g)", r2);
    if (n_clouds == 0 || total_points == 0) return SGA_OK;
    SGA_CHECK_ARG(pts && cell && origin && dims && status && order && sorted_keys && count && idx && d2, "sga_knn_lists_grid: null pointer");
    SGA_CHECK_ARG(sga_aligned(8, pts, cell, origin, sorted_keys, d2) && sga_aligned(4, dims, status, order, count, idx),
                  "sga_knn_lists_grid: misaligned pointer (fp64 and int64 arrays need 8 bytes, int32 arrays 4)");
    const long grid = ((long)total_points + KL_WAVES - 1) / KL_WAVES;
    if (int rc = sga_check_grid("sga_knn_lists_grid", grid, 1, 1, "split the cloud list")) return rc;
    hipLaunchKernelGGL(vg_knn_kernel, dim3((unsigned)grid), dim3(KL_THREADS), 0, static_cast<hipStream_t>(stream), pts, offsets, n_clouds,
                       total_points, cell, origin, dims, status, order, reinterpret_cast<const long long*>(sorted_keys), r2, max_nn, count, idx, d2);
    SGA_CHECK_LAUNCH("sga_knn_lists_grid");
    return SGA_OK;
}
