// FPFH descriptors on the device: exact k-NN / radius neighbour lists, normals, the SPFH census and the FPFH weighting, batched over clouds.
//
// The descriptor side of utils/open3d.py:61-66 (estimate_normals), :78-86 and :137-170 (FPFH features into feature-matching RANSAC): the
// chain  points -> neighbour lists -> normals -> SPFH -> FPFH  that feeds csrc/featnn.hip and csrc/ransac.hip.  Open3D itself is not a
// dependency; the contract written in include/sgaligner_hip.h IS the definition, and tests/fpfh_ref.py restates it in numpy.
//
// Clouds are packed back to back (csrc/packed.h): pts [total_points, 3] f64, offsets [n_clouds + 1].  Neighbours are always taken from the
// point's own cloud and indices are cloud-local.  Every kernel re-checks each offset, count and index it reads: a bad one makes it do
// nothing (or skip that neighbour), never read or write out of bounds.  No floating-point atomics anywhere: every output is a pure function
// of the input.
//
// knn_kernel (the hot path): brute force, one wave per query, four queries per workgroup.  The cloud streams through an SoA LDS tile of
// 512 points (3 x 4 KiB; lane l reads point s + l: consecutive 8-byte addresses, no bank conflict), lane l evaluates
// d2 = (dx*dx + dy*dy) + dz*dz for support point t0 + s + l -- the arithmetic of nnsearch.hip, each operation rounded on its own (explicit
// __d*_rn forms AND -ffp-contract=off for this file).  A candidate is admitted iff d2 <= r2 and, once the list is full, d2 < tau, tau the
// current max_nn-th best d2.  Strict <: the walk ascends in j, so an equal d2 that arrives later has the larger index and loses.  Admitted
// candidates are compacted with __ballot / popcount behind the wave's list in LDS (up to 64 staged entries); when a ballot does not fit,
// the <= 128 + 64 (d2, j) pairs are rank-sorted in place -- each lane counts the entries lexicographically smaller than its own (at most
// three per lane, in named registers; the list is sorted already, so only the staged entries are walked and a staged entry finds its place
// in the list by a binary search) and writes them at that rank -- the first max_nn are kept and tau is refreshed.  Admission against a
// stale tau is merely conservative, so the result does not depend on when the merges happen.  About 11 fp64 VALU operations per pair; the
// merges are the smaller part of the time.  LDS: 12 KiB tile + 4 x 192 x 12 B lists = 21 KiB per workgroup.
// Workgroup -> (cloud, query tile): tile t of cloud c has id (offsets[c] >> 2) + c + t, found by a search over `offsets`; at most one
// workgroup per cloud is left without work.
//
// normals_kernel / fpfh_kernel: one lane per point (per point and bin group); sums run in list order, so they are sequential by contract.
// spfh_kernel: one wave per point, lane k takes list entry 1 + k; the 33 bins are integer LDS atomics (integer sums do not depend on order).
#include "pair_jobs.h"
#include "wave_search.h"

namespace {

constexpr int KL_THREADS = 256;
constexpr int KL_WAVES = 4;                        // queries per workgroup: one wave each
constexpr int KL_STILE = 512;                      // support points per LDS tile (12 KiB)
constexpr int KL_MAX_NN = 128;                     // longest list
constexpr int KL_STAGE = 64;                       // staged candidates per wave: one full ballot
constexpr int KL_SLOTS = KL_MAX_NN + KL_STAGE;     // entries a merge sorts, three per lane at most
constexpr int FP_BINS = 33;
constexpr int NR_SWEEPS = 8;                       // cyclic Jacobi sweeps on the 3x3 covariance: always this many (it converges in 4-5)
constexpr double FP_PI = 3.14159265358979323846;

// knn_kernel's list state around kl_rank_sort (wave_search.h), its staged-entry loop unrolled by 2; refreshes tau once the list is full.
__device__ __forceinline__ void kl_merge(double* __restrict__ wd, int* __restrict__ wi, int lane, int max_nn, int& L, int& S, double& tau,
                                         bool& full) {
    const int E = L + S;
    sga_wave_sync();
    if (E <= 64) kl_rank_sort<1, 2>(wd, wi, lane, L, E, max_nn);
    else if (E <= 128) kl_rank_sort<2, 2>(wd, wi, lane, L, E, max_nn);
    else kl_rank_sort<3, 2>(wd, wi, lane, L, E, max_nn);
    L = min(E, max_nn);
    S = 0;
    if (E >= max_nn) { full = true; tau = wd[max_nn - 1]; }
}

__global__ __launch_bounds__(KL_THREADS) void knn_kernel(const double* __restrict__ pts, const int* __restrict__ off, int n_clouds,
                                                         int total_points, double r2, int max_nn, int* __restrict__ out_count,
                                                         int* __restrict__ out_idx, double* __restrict__ out_d2) {
    __shared__ double sx[KL_STILE], sy[KL_STILE], sz[KL_STILE];
    __shared__ double list_d[KL_WAVES][KL_SLOTS];
    __shared__ int list_i[KL_WAVES][KL_SLOTS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.x;
    // the last cloud whose first tile id (offsets[c] >> 2) + c is <= b
    int lo = 0, hi = n_clouds - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if ((off[mid] >> 2) + mid <= b) lo = mid; else hi = mid - 1;
    }
    const SgaCloud C = sga_cloud(off, total_points, lo);
    if (!C.ok) return;
    const long long t = (long long)b - ((C.o0 >> 2) + lo);
    if (t < 0 || t * KL_WAVES >= C.n) return;                   // before the first cloud's tiles, or the spare id between two clouds
    const int q = (int)t * KL_WAVES + wave;                     // this wave's query, cloud-local
    const bool active = q < C.n;
    const double* P = pts + (size_t)C.o0 * 3;
    const double qx = active ? P[(size_t)q * 3 + 0] : 0.0, qy = active ? P[(size_t)q * 3 + 1] : 0.0, qz = active ? P[(size_t)q * 3 + 2] : 0.0;
    double* wd = list_d[wave];
    int* wi = list_i[wave];
    int L = 0, S = 0;                                           // list length, staged entries: wave-uniform
    double tau = INFINITY;
    bool full = false;
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int t0 = 0; t0 < C.n; t0 += KL_STILE) {
        const int m = min(KL_STILE, C.n - t0);
        __syncthreads();                                        // the previous tile has been consumed by every wave
        for (int j = tid; j < m; j += KL_THREADS) {
            sx[j] = P[(size_t)(t0 + j) * 3 + 0];
            sy[j] = P[(size_t)(t0 + j) * 3 + 1];
            sz[j] = P[(size_t)(t0 + j) * 3 + 2];
        }
        __syncthreads();
        if (!active) continue;
        for (int s = 0; s < m; s += 64) {
            const int jj = s + lane;
            const bool inb = jj < m;
            const int jr = inb ? jj : 0;
            const double dx = __dsub_rn(qx, sx[jr]), dy = __dsub_rn(qy, sy[jr]), dz = __dsub_rn(qz, sz[jr]);
            const double d2 = __dadd_rn(__dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)), __dmul_rn(dz, dz));
            bool adm = inb && d2 <= r2 && (!full || d2 < tau);  // a NaN fails d2 <= r2
            unsigned long long bal = __ballot(adm);
            if (bal == 0ull) continue;
            int c = __popcll(bal);
            if (S + c > KL_STAGE) {
                kl_merge(wd, wi, lane, max_nn, L, S, tau, full);
                adm = adm && (!full || d2 < tau);
                bal = __ballot(adm);
                c = __popcll(bal);
            }
            if (adm) {
                const int slot = L + S + __popcll(bal & below); // < max_nn + 64
                wd[slot] = d2;
                wi[slot] = t0 + jj;
            }
            S += c;
        }
    }
    if (!active) return;
    if (S > 0) kl_merge(wd, wi, lane, max_nn, L, S, tau, full);
    sga_wave_sync();
    const size_t row = ((size_t)C.o0 + q) * max_nn;
    for (int e = lane; e < max_nn; e += 64) {
        out_idx[row + e] = e < L ? wi[e] : -1;
        out_d2[row + e] = e < L ? wd[e] : INFINITY;
    }
    if (lane == 0) out_count[(size_t)C.o0 + q] = L;
}

// ---- normals ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void normals_kernel(const double* __restrict__ pts, const int* __restrict__ off, int n_clouds, int total_points,
                                                      const int* __restrict__ count, const int* __restrict__ idx, int max_nn,
                                                      const double* __restrict__ viewpoints, double* __restrict__ normals,
                                                      int* __restrict__ status) {
    const long long gi = (long long)blockIdx.x * 256 + threadIdx.x;
    if (gi >= total_points) return;
    const int i = (int)gi;
    const SgaCloud C = sga_cloud_of_point(off, n_clouds, total_points, i);
    if (!C.ok) return;
    const double* P = pts + (size_t)C.o0 * 3;
    const int* row = idx + (size_t)i * max_nn;
    const int m = count[i];
    const double px = pts[(size_t)i * 3], py = pts[(size_t)i * 3 + 1], pz = pts[(size_t)i * 3 + 2];
    bool good = m >= 3 && m <= max_nn && isfinite(px) && isfinite(py) && isfinite(pz);
    double mx = 0.0, my = 0.0, mz = 0.0;
    for (int k = 0; good && k < m; ++k) {
        const int j = row[k];
        if (j < 0 || j >= C.n) { good = false; break; }
        const double x = P[(size_t)j * 3], y = P[(size_t)j * 3 + 1], z = P[(size_t)j * 3 + 2];
        if (!(isfinite(x) && isfinite(y) && isfinite(z))) { good = false; break; }
        mx += x; my += y; mz += z;
    }
    double nx = 0.0, ny = 0.0, nz = 1.0;
    if (good) {
        const double dm = (double)m;
        mx /= dm; my /= dm; mz /= dm;
        double cxx = 0.0, cxy = 0.0, cxz = 0.0, cyy = 0.0, cyz = 0.0, czz = 0.0;
        for (int k = 0; k < m; ++k) {
            const int j = row[k];
            const double x = P[(size_t)j * 3] - mx, y = P[(size_t)j * 3 + 1] - my, z = P[(size_t)j * 3 + 2] - mz;
            cxx += x * x; cxy += x * y; cxz += x * z; cyy += y * y; cyz += y * z; czz += z * z;
        }
        double A[3][3], V[3][3];
        A[0][0] = cxx / dm; A[1][1] = cyy / dm; A[2][2] = czz / dm;
        A[0][1] = A[1][0] = cxy / dm; A[0][2] = A[2][0] = cxz / dm; A[1][2] = A[2][1] = cyz / dm;
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int c = 0; c < 3; ++c) V[a][c] = a == c ? 1.0 : 0.0;
#pragma unroll 1
        for (int sweep = 0; sweep < NR_SWEEPS; ++sweep) {
#pragma unroll
            for (int p = 0; p < 2; ++p) {
#pragma unroll
                for (int q = p + 1; q < 3; ++q) {
                    const double apq = A[p][q];
                    if (apq == 0.0) continue;                            // nothing to rotate: the pair stays exactly as it is
                    const double theta = (A[q][q] - A[p][p]) / (2.0 * apq);
                    const double tt = (theta < 0.0 ? -1.0 : 1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));      // |theta| huge: 1 / inf = 0
                    const double c = 1.0 / sqrt(tt * tt + 1.0), s = tt * c;
                    A[p][p] -= tt * apq;
                    A[q][q] += tt * apq;
                    A[p][q] = A[q][p] = 0.0;
#pragma unroll
                    for (int k = 0; k < 3; ++k) {
                        if (k != p && k != q) {
                            const double akp = A[k][p], akq = A[k][q];
                            A[k][p] = A[p][k] = c * akp - s * akq;
                            A[k][q] = A[q][k] = s * akp + c * akq;
                        }
                        const double vkp = V[k][p], vkq = V[k][q];
                        V[k][p] = c * vkp - s * vkq;
                        V[k][q] = s * vkp + c * vkq;
                    }
                }
            }
        }
        double lam = A[0][0];
        nx = V[0][0]; ny = V[1][0]; nz = V[2][0];
#pragma unroll
        for (int c = 1; c < 3; ++c)
            if (A[c][c] < lam) { lam = A[c][c]; nx = V[0][c]; ny = V[1][c]; nz = V[2][c]; }      // strict: the lowest column among equal eigenvalues
        const double len = sqrt((nx * nx + ny * ny) + nz * nz);
        nx /= len; ny /= len; nz /= len;
        if (!(isfinite(nx) && isfinite(ny) && isfinite(nz))) {
            good = false;
            nx = 0.0; ny = 0.0; nz = 1.0;
        }
    }
    if (good) {
        bool flip;
        if (viewpoints) {
            const double vx = viewpoints[(size_t)C.c * 3] - px, vy = viewpoints[(size_t)C.c * 3 + 1] - py, vz = viewpoints[(size_t)C.c * 3 + 2] - pz;
            flip = (nx * vx + ny * vy) + nz * vz < 0.0;
        } else {
            const double ax = fabs(nx), ay = fabs(ny), az = fabs(nz);
            const double big = (ax >= ay && ax >= az) ? nx : (ay >= az ? ny : nz);            // lowest axis among equal magnitudes
            flip = big < 0.0;
        }
        if (flip) { nx = -nx; ny = -ny; nz = -nz; }
    }
    normals[(size_t)i * 3] = nx;
    normals[(size_t)i * 3 + 1] = ny;
    normals[(size_t)i * 3 + 2] = nz;
    status[i] = good ? 0 : 1;
}

// ---- SPFH census -----------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int fp_bin(double t) {                // floor(t) clamped to [0, 10]; NaN -> 0
    return t >= 0.0 ? (t >= 10.0 ? 10 : (int)floor(t)) : 0;
}

__global__ __launch_bounds__(256) void spfh_kernel(const double* __restrict__ pts, const double* __restrict__ normals, const int* __restrict__ off,
                                                   int n_clouds, int total_points, const int* __restrict__ count, const int* __restrict__ idx,
                                                   const double* __restrict__ d2, int max_nn, int* __restrict__ counts) {
    __shared__ int bins[4][FP_BINS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long gi = (long long)blockIdx.x * 4 + wave;
    if (gi >= total_points) return;                              // no workgroup-wide barrier below: a wave may leave on its own
    const int i = (int)gi;
    const SgaCloud C = sga_cloud_of_point(off, n_clouds, total_points, i);
    if (!C.ok) return;
    if (lane < FP_BINS) bins[wave][lane] = 0;
    sga_wave_sync();
    const int mc = count[i];
    const int m = mc < 0 ? 0 : (mc > max_nn ? max_nn : mc);
    const double* P = pts + (size_t)C.o0 * 3;
    const double* N = normals + (size_t)C.o0 * 3;
    const double p1x = pts[(size_t)i * 3], p1y = pts[(size_t)i * 3 + 1], p1z = pts[(size_t)i * 3 + 2];
    const double m1x = normals[(size_t)i * 3], m1y = normals[(size_t)i * 3 + 1], m1z = normals[(size_t)i * 3 + 2];
    for (int k = 1 + lane; k < m; k += 64) {
        const int j = idx[(size_t)i * max_nn + k];
        if (j < 0 || j >= C.n) continue;                         // skipped, never read
        const double d = sqrt(d2[(size_t)i * max_nn + k]);
        double f0 = 0.0, f1 = 0.0, f2 = 0.0;
        if (!(d == 0.0)) {
            double n1x = m1x, n1y = m1y, n1z = m1z;
            double n2x = N[(size_t)j * 3], n2y = N[(size_t)j * 3 + 1], n2z = N[(size_t)j * 3 + 2];
            double dpx = P[(size_t)j * 3] - p1x, dpy = P[(size_t)j * 3 + 1] - p1y, dpz = P[(size_t)j * 3 + 2] - p1z;
            const double a1 = ((n1x * dpx + n1y * dpy) + n1z * dpz) / d, a2 = ((n2x * dpx + n2y * dpy) + n2z * dpz) / d;
            double g2;
            if (fabs(a1) < fabs(a2)) {
                double tx = n1x, ty = n1y, tz = n1z;
                n1x = n2x; n1y = n2y; n1z = n2z;
                n2x = tx; n2y = ty; n2z = tz;
                dpx = -dpx; dpy = -dpy; dpz = -dpz;
                g2 = -a2;
            } else {
                g2 = a1;
            }
            double vx = dpy * n1z - dpz * n1y, vy = dpz * n1x - dpx * n1z, vz = dpx * n1y - dpy * n1x;
            const double vn = sqrt((vx * vx + vy * vy) + vz * vz);
            if (!(vn == 0.0)) {
                vx /= vn; vy /= vn; vz /= vn;
                const double wx = n1y * vz - n1z * vy, wy = n1z * vx - n1x * vz, wz = n1x * vy - n1y * vx;
                f1 = (vx * n2x + vy * n2y) + vz * n2z;
                f0 = atan2((wx * n2x + wy * n2y) + wz * n2z, (n1x * n2x + n1y * n2y) + n1z * n2z);
                f2 = g2;
            }
        }
        atomicAdd(&bins[wave][fp_bin(11.0 * (f0 + FP_PI) / (2.0 * FP_PI))], 1);
        atomicAdd(&bins[wave][11 + fp_bin(11.0 * (f1 + 1.0) / 2.0)], 1);
        atomicAdd(&bins[wave][22 + fp_bin(11.0 * (f2 + 1.0) / 2.0)], 1);
    }
    sga_wave_sync();
    if (lane < FP_BINS) counts[(size_t)i * FP_BINS + lane] = bins[wave][lane];
}

// ---- FPFH weighting --------------------------------------------------------------------------------------------------------------------
// 100 / (m - 1) of point x, 0 for a list of at most one entry
__device__ __forceinline__ double fp_scale(int m) { return m > 1 ? 100.0 / (double)(m - 1) : 0.0; }

__global__ __launch_bounds__(256) void fpfh_kernel(const int* __restrict__ counts, const int* __restrict__ off, int n_clouds, int total_points,
                                                   const int* __restrict__ count, const int* __restrict__ idx, const double* __restrict__ d2,
                                                   int max_nn, double* __restrict__ out64, float* __restrict__ out32, int ld) {
    const long long gt = (long long)blockIdx.x * 256 + threadIdx.x;
    if (gt >= 3ll * total_points) return;
    const int i = (int)(gt / 3), g = (int)(gt % 3);
    const SgaCloud C = sga_cloud_of_point(off, n_clouds, total_points, i);
    if (!C.ok) return;
    const int mc = count[i];
    const int m = mc < 0 ? 0 : (mc > max_nn ? max_nn : mc);
    double acc[11];
#pragma unroll
    for (int c = 0; c < 11; ++c) acc[c] = 0.0;
    double sum = 0.0;
    for (int k = 1; k < m; ++k) {
        const int j = idx[(size_t)i * max_nn + k];
        const double dk = d2[(size_t)i * max_nn + k];
        if (j < 0 || j >= C.n || dk == 0.0) continue;
        const int mj = count[C.o0 + j];
        const double sc = fp_scale(mj < 0 ? 0 : (mj > max_nn ? max_nn : mj));
        const int* cj = counts + ((size_t)C.o0 + j) * FP_BINS + g * 11;
#pragma unroll
        for (int c = 0; c < 11; ++c) {
            const double val = ((double)cj[c] * sc) / dk;
            sum += val;
            acc[c] += val;
        }
    }
    const double si = fp_scale(m), w = sum != 0.0 ? 100.0 / sum : 1.0;
    const int* ci = counts + (size_t)i * FP_BINS + g * 11;
#pragma unroll
    for (int c = 0; c < 11; ++c) {
        const double a = sum != 0.0 ? acc[c] * w : acc[c];
        const double v = a + (double)ci[c] * si;
        if (out64) out64[(size_t)i * FP_BINS + g * 11 + c] = v;
        out32[(size_t)i * ld + g * 11 + c] = (float)v;
    }
    if (g == 2)
        for (int c = FP_BINS; c < ld; ++c) out32[(size_t)i * ld + c] = 0.0f;
}

// What the four entries check alike: counts, the list width, the offsets' host copy.
int fp_check(const char* who, const void* offsets, int n_clouds, int total_points, const int32_t* offsets_host, int max_nn) {
    SGA_CHECK_ARG(n_clouds >= 0 && total_points >= 0, "%s: negative count (n_clouds %d, total_points %d)", who, n_clouds, total_points);
    SGA_CHECK_ARG(max_nn >= 1 && max_nn <= KL_MAX_NN, "%s: max_nn must be in [1, %d] (got %d)", who, KL_MAX_NN, max_nn);
    SGA_CHECK_ARG((long long)total_points * max_nn < (1LL << 31), "%s: total_points x max_nn must stay below 2^31 (%d x %d)", who, total_points, max_nn);
    const SgaPrefix OFFSETS{"offsets", "decrease", "cloud", "total_points", nullptr, nullptr};
    if (int rc = sga_check_prefix(who, OFFSETS, offsets_host, n_clouds, total_points, SGA_ANY)) return rc;
    SGA_CHECK_ARG(offsets || n_clouds == 0 || total_points == 0, "%s: null offsets", who);
    SGA_CHECK_ARG(sga_aligned(4, offsets), "%s: misaligned offsets (int32 arrays need 4 bytes)", who);
    return SGA_OK;
}

}  // namespace

extern "C" int sga_knn_lists(const double* pts, const int32_t* offsets, int n_clouds, int total_points, const int32_t* offsets_host, double r2,
                             int max_nn, int32_t* count, int32_t* idx, double* d2, void* stream) {
    if (int rc = fp_check("sga_knn_lists", offsets, n_clouds, total_points, offsets_host, max_nn)) return rc;
    SGA_CHECK_ARG(r2 >= 0.0, "sga_knn_lists: r2 must be >= 0 or +inf (got %g)", r2);
    if (n_clouds == 0 || total_points == 0) return SGA_OK;
    SGA_CHECK_ARG(pts && count && idx && d2, "sga_knn_lists: null pointer");
    SGA_CHECK_ARG(sga_aligned(8, pts, d2) && sga_aligned(4, count, idx), "sga_knn_lists: misaligned pointer (fp64 arrays need 8 bytes, int32 arrays 4)");
    const long grid = (long)(total_points / KL_WAVES) + n_clouds;
    if (int rc = sga_check_grid("sga_knn_lists", grid, 1, 1, "split the cloud list")) return rc;
    hipLaunchKernelGGL(knn_kernel, dim3((unsigned)grid), dim3(KL_THREADS), 0, static_cast<hipStream_t>(stream), pts, offsets, n_clouds, total_points,
                       r2, max_nn, count, idx, d2);
    SGA_CHECK_LAUNCH("sga_knn_lists");
    return SGA_OK;
}

extern "C" int sga_normals(const double* pts, const int32_t* offsets, int n_clouds, int total_points, const int32_t* offsets_host,
                           const int32_t* count, const int32_t* idx, int max_nn, const double* viewpoints, double* normals, int32_t* status,
                           void* stream) {
    if (int rc = fp_check("sga_normals", offsets, n_clouds, total_points, offsets_host, max_nn)) return rc;
    if (n_clouds == 0 || total_points == 0) return SGA_OK;
    SGA_CHECK_ARG(pts && count && idx && normals && status, "sga_normals: null pointer");
    SGA_CHECK_ARG(sga_aligned(8, pts, viewpoints, normals) && sga_aligned(4, count, idx, status),
                  "sga_normals: misaligned pointer (fp64 arrays need 8 bytes, int32 arrays 4)");
    const long grid = ((long)total_points + 255) / 256;
    hipLaunchKernelGGL(normals_kernel, dim3((unsigned)grid), dim3(256), 0, static_cast<hipStream_t>(stream), pts, offsets, n_clouds, total_points,
                       count, idx, max_nn, viewpoints, normals, status);
    SGA_CHECK_LAUNCH("sga_normals");
    return SGA_OK;
}

extern "C" int sga_spfh_counts(const double* pts, const double* normals, const int32_t* offsets, int n_clouds, int total_points,
                               const int32_t* offsets_host, const int32_t* count, const int32_t* idx, const double* d2, int max_nn,
                               int32_t* counts, void* stream) {
    if (int rc = fp_check("sga_spfh_counts", offsets, n_clouds, total_points, offsets_host, max_nn)) return rc;
    if (n_clouds == 0 || total_points == 0) return SGA_OK;
    SGA_CHECK_ARG(pts && normals && count && idx && d2 && counts, "sga_spfh_counts: null pointer");
    SGA_CHECK_ARG(sga_aligned(8, pts, normals, d2) && sga_aligned(4, count, idx, counts),
                  "sga_spfh_counts: misaligned pointer (fp64 arrays need 8 bytes, int32 arrays 4)");
    const long grid = ((long)total_points + 3) / 4;
    hipLaunchKernelGGL(spfh_kernel, dim3((unsigned)grid), dim3(256), 0, static_cast<hipStream_t>(stream), pts, normals, offsets, n_clouds,
                       total_points, count, idx, d2, max_nn, counts);
    SGA_CHECK_LAUNCH("sga_spfh_counts");
    return SGA_OK;
}

extern "C" int sga_fpfh(const int32_t* counts, const int32_t* offsets, int n_clouds, int total_points, const int32_t* offsets_host,
                        const int32_t* count, const int32_t* idx, const double* d2, int max_nn, double* out64, float* out32, int ld, void* stream) {
    if (int rc = fp_check("sga_fpfh", offsets, n_clouds, total_points, offsets_host, max_nn)) return rc;
    SGA_CHECK_ARG(ld >= FP_BINS && ld % 4 == 0, "sga_fpfh: ld must be >= %d and a multiple of 4 (got %d)", FP_BINS, ld);
    SGA_CHECK_ARG((long long)total_points * ld < (1LL << 31), "sga_fpfh: total_points x ld must stay below 2^31 (%d x %d)", total_points, ld);
    if (n_clouds == 0 || total_points == 0) return SGA_OK;
    SGA_CHECK_ARG(counts && count && idx && d2 && out32, "sga_fpfh: null pointer");
    SGA_CHECK_ARG(sga_aligned(8, d2, out64) && sga_aligned(4, counts, count, idx, out32),
                  "sga_fpfh: misaligned pointer (fp64 arrays need 8 bytes, int32 and fp32 arrays 4)");
    const long grid = (3L * total_points + 255) / 256;
    hipLaunchKernelGGL(fpfh_kernel, dim3((unsigned)grid), dim3(256), 0, static_cast<hipStream_t>(stream), counts, offsets, n_clouds, total_points,
                       count, idx, d2, max_nn, out64, out32, ld);
    SGA_CHECK_LAUNCH("sga_fpfh");
    return SGA_OK;
}
