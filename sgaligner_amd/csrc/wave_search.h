// What the one-wave-per-query searches share: knn_kernel (fpfh.hip), vg_knn_kernel (voxel.hip), icp_nn_grid_kernel (icp.hip) and gs_search
// under geo_score_kernel (ransac_geo.hip).  The grid constants, the wave-level helpers and the rank-sort merge of the k-NN list stand here
// once; the contracts of include/sgaligner_hip.h promise results bit for bit, and the proofs of the stop rule (heads of voxel.hip and
// icp.hip) lean on these exact expressions.  The grid WALK itself is not here: the three walks differ on purpose in where values are held
// (see the comment above geo_score_kernel).
#pragma once
#include <limits.h>
#include <math.h>

#include "sga_common.h"

// ---- the cell grid of sga_voxel_keys / sga_voxel_cells ---------------------------------------------------------------------------------------
constexpr int GRID_DROPPED = 65535;                // the cell coordinate of a dropped point; a valid one is below it
constexpr int GRID_MAX_CLOUDS = 32767;             // the cloud id is the key's top field: 15 bits keep the key non-negative
constexpr int GRID_MAX_R = 16;                     // block radii 1, 2, 4, 8, 16; then the whole cloud
constexpr double GRID_EPS = 0x1p-40;               // the margin of the stop rule

// ---- wave helpers ----------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void sga_wave_sync() {    // the wave's own LDS writes before its next LDS reads: lanes exchange entries
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// (d2, j) order: the lowest index among exactly equal distances wins whatever the order candidates arrive in.
__device__ __forceinline__ bool sga_d2j_less(double da, int ja, double db, int jb) { return da < db || (da == db && ja < jb); }

// (dx dx + dy dy) + dz dz, every operation rounded on its own: the d2 of nnsearch.hip and knn_kernel.
__device__ __forceinline__ double sga_point_d2(double qx, double qy, double qz, const double* __restrict__ p) {
    const double dx = __dsub_rn(qx, p[0]), dy = __dsub_rn(qy, p[1]), dz = __dsub_rn(qz, p[2]);
    return __dadd_rn(__dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)), __dmul_rn(dz, dz));
}

// The lane's candidate against the lane's best: within r2, below +inf (nn_kernel's strict < against its +inf start), a NaN fails both.
__device__ __forceinline__ void sga_nn_offer(double r2, double d2, int j, bool live, double& bd, int& bj) {
    if (live && d2 <= r2 && d2 < INFINITY && sga_d2j_less(d2, j, bd, bj)) { bd = d2; bj = j; }
}

// The wave's best (d2, j), to every lane.
__device__ __forceinline__ void sga_wave_best(double& bd, int& bj) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double od = __shfl_xor(bd, o, 64);
        const int oj = __shfl_xor(bj, o, 64);
        if (sga_d2j_less(od, oj, bd, bj)) { bd = od; bj = oj; }
    }
}

// first position of sk[0, n) whose key is >= key
__device__ __forceinline__ int sga_lower_bound(const long long* __restrict__ sk, int n, long long key) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (sk[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// The search's move of a point, one coordinate: ((m[3 row] x + m[3 row + 1] y) + m[3 row + 2] z) + m[9 + row], no fma.
__device__ __forceinline__ double sga_move_point(const double* __restrict__ m, int row, double x, double y, double z) {
    return __dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(m[3 * row], x), __dmul_rn(m[3 * row + 1], y)), __dmul_rn(m[3 * row + 2], z)), m[9 + row]);
}

// ---- the k-NN list's merge -------------------------------------------------------------------------------------------------------------------
// Merge the wave's S staged entries [L, L + S) into its sorted list [0, L) in place and keep the first max_nn: a rank sort in which only the
// staged entries are walked.  An entry's rank is the number of entries below it by (d2, j): for a list entry its own position plus the
// staged entries below it; for a staged entry the staged entries below it plus its lower bound in the sorted list (a binary search).
// E = L + S <= 64 * K; every lane holds at most K entries in named registers.  UNROLL is the unroll count of the staged-entry loop, the
// caller's choice by its register budget: knn_kernel takes 2 (4 keeps too many compare masks alive: the scalar registers spill),
// vg_knn_kernel 1.
template <int K, int UNROLL>
__device__ __forceinline__ void kl_rank_sort(double* __restrict__ wd, int* __restrict__ wi, int lane, int L, int E, int max_nn) {
    double d[K];
    int j[K], r[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int e = lane + 64 * k;
        const bool ok = e < E;
        d[k] = ok ? wd[e] : INFINITY;
        j[k] = ok ? wi[e] : INT_MAX;
        r[k] = e < L ? e : 0;
    }
#pragma unroll UNROLL
    for (int m = L; m < E; ++m) {
        const double dm = wd[m];                     // one address for the whole wave: broadcast
        const int jm = wi[m];
#pragma unroll
        for (int k = 0; k < K; ++k) r[k] += sga_d2j_less(dm, jm, d[k], j[k]) ? 1 : 0;
    }
#pragma unroll
    for (int k = 0; k < K; ++k) {
        if (L >= 64 * (k + 1) || E <= 64 * k || L == 0) continue;                  // wave-uniform: no staged entry among these 64, or no list
        const int e = lane + 64 * k;
        int lo = 0, hi = (e >= L && e < E) ? L : 0;                                 // staged entries only; L <= 128: 8 halvings
#pragma unroll 1
        for (int step = 0; step < 8; ++step) {                                      // branch-free: every lane walks all steps
            const int mid = (lo + hi) >> 1;                                         // < L whenever lo < hi; else lo == hi <= L
            const int at = min(mid, L - 1);
            const bool go = lo < hi, up = sga_d2j_less(wd[at], wi[at], d[k], j[k]);
            lo = (go && up) ? mid + 1 : lo;
            hi = (go && !up) ? mid : hi;
        }
        r[k] += lo;
    }
    sga_wave_sync();                                 // every lane has read before any lane writes
#pragma unroll
    for (int k = 0; k < K; ++k)
        if (lane + 64 * k < E && r[k] < max_nn) { wd[r[k]] = d[k]; wi[r[k]] = j[k]; }      // (d2, j) pairs are distinct: the ranks are a permutation
    sga_wave_sync();
}
