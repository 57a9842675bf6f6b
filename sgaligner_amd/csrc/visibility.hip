// Batched subscan generation: per-frame point visibility, the frame walk that closes subscans, and per-object visible-point counts.
//
// Replaces the per-frame NumPy / OpenCV loop of preprocessing/scan3r/subgenscan3r.py:188-234: get_visible_pts_from_cam_pose
// (utils/point_cloud.py:112-134) for every frame of a scan, the running OR of the masks with a subscan closed whenever the union reaches
// the point budget, and the per-object counts gen_scene_graph (:51-85) thresholds the relationships with.
//
// Scans are packed back to back: pts [sum N, 3] f32 / pt_off [S + 1], w2c [sum F, 12] f64 (rows 0-2 of the world-to-camera matrix, row-major)
// / fr_off [S + 1], intr [S, 6] f64 = fx, fy, cx, cy, u_max, v_max.  Scan s owns a bit matrix of F_s rows by W_s = ceil(N_s / 64) 64-bit
// words starting at word vis_off[s]; bit p % 64 of word p / 64 of a row is point p, the padding bits of the last word are 0.
//
// Arithmetic contract of the visibility test, every fp64 operation rounded on its own (the explicit __d*_rn forms AND -ffp-contract=off
// for this file, _build.FILE_FLAGS), x, y, z the f32 vertex widened to f64:
//     X = ((x*m00 + y*m01) + z*m02) + m03       (Y, Z with rows 1, 2)
//     r = (Z != 0) ? 1.0 / Z : 1.0              (correctly rounded division)
//     u = (X*r)*fx + cx ;  v = (Y*r)*fy + cy
//     visible = (Z > 0) && (u >= 0) && (u <= u_max) && (v >= 0) && (v <= v_max)
// Every comparison is false on a NaN, so a NaN anywhere (coordinate, pose, intrinsics) gives "invisible".
//
// vis_kernel: one lane per point (VIS_PPL points per lane), a group of VIS_FG frames per workgroup with the frame's parameters wave-uniform,
// one __ballot (64 bits on this wave size) per frame, wave and point slot; the words are staged in LDS and leave as VIS_WORDS contiguous
// words per frame row.  walk_kernel: one workgroup per scan, sequential over its frames, parallel over words; the running union IS the
// previous row of `cum` (or nothing after a closed subscan), so `cum` may be `vis` itself.  objcount_kernel: one lane per point of a bit row,
// a workgroup-private LDS histogram flushed with integer atomics (global integer atomics above VIS_LDS_SLOTS slots): exact, order-independent.
// All three re-derive the scan's ranges from the device offset arrays and do nothing on a bad one.
#include "packed.h"

namespace {

typedef unsigned long long u64;

constexpr int VIS_THREADS = 256;
constexpr int VIS_PPL = 4;                                   // points per lane: 12 fp64 coordinates in registers
constexpr int VIS_WORDS = (VIS_THREADS / 64) * VIS_PPL;      // 64-bit words a workgroup writes per frame row (128 contiguous bytes)
constexpr int VIS_PTILE = VIS_WORDS * 64;                    // points per workgroup
constexpr int VIS_FG = VIS_THREADS / VIS_WORDS;              // frames per workgroup: one staged word per lane at the write-out
constexpr int WALK_THREADS = 1024;
constexpr int OC_THREADS = 256;
constexpr int OC_PPL = 16;
constexpr int OC_TILE = OC_THREADS * OC_PPL;                 // points of a bit row per workgroup
constexpr int VIS_LDS_SLOTS = 1024;                          // largest n_slots served by the LDS histogram (4 KiB)

struct VScan { int p0, n, f0, nf; long long v0, W; bool ok; };

// Everything a workgroup needs to know about scan `s`, read from the device arrays and range-checked: a bad offset makes the workgroup
// do nothing instead of reading or writing out of bounds.
__device__ __forceinline__ VScan vis_scan(const int* __restrict__ pt_off, const int* __restrict__ fr_off, const long long* __restrict__ vis_off,
                                          int n_scans, int total_points, int total_frames, long long total_words, int s) {
    VScan S{0, 0, 0, 0, 0, 0, false};
    if (s < 0 || s >= n_scans) return S;
    const int p0 = pt_off[s], p1 = pt_off[s + 1], f0 = fr_off[s], f1 = fr_off[s + 1];
    const long long v0 = vis_off[s];
    if (p0 < 0 || p1 < p0 || p1 > total_points || f0 < 0 || f1 < f0 || f1 > total_frames) return S;
    const long long W = ((long long)(p1 - p0) + 63) / 64;
    if (v0 < 0 || v0 > total_words || (long long)(f1 - f0) * W > total_words - v0) return S;
    return VScan{p0, p1 - p0, f0, f1 - f0, v0, W, true};
}

__global__ __launch_bounds__(VIS_THREADS) void vis_kernel(const float* __restrict__ pts, const int* __restrict__ pt_off,
                                                          const double* __restrict__ w2c, const int* __restrict__ fr_off,
                                                          const double* __restrict__ intr, const long long* __restrict__ vis_off, int n_scans,
                                                          int total_points, int total_frames, long long total_words, int p_tiles, int f_groups,
                                                          u64* __restrict__ vis) {
    __shared__ u64 sw[VIS_FG][VIS_WORDS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int b = blockIdx.x;
    const int pt = b % p_tiles;
    b /= p_tiles;
    const int fg = b % f_groups, s = b / f_groups;
    const VScan S = vis_scan(pt_off, fr_off, vis_off, n_scans, total_points, total_frames, total_words, s);
    if (!S.ok) return;
    const long long pb = (long long)pt * VIS_PTILE;
    const int fb = fg * VIS_FG;
    if (pb >= S.n || fb >= S.nf) return;
    const int nfr = min(VIS_FG, S.nf - fb);

    const float* P = pts + (size_t)S.p0 * 3;
    double x[VIS_PPL], y[VIS_PPL], z[VIS_PPL];
    bool in[VIS_PPL];
#pragma unroll
    for (int k = 0; k < VIS_PPL; ++k) {                      // word (wave * VIS_PPL + k) of the tile, bit `lane`
        const long long i = pb + (wave * VIS_PPL + k) * 64 + lane;
        in[k] = i < S.n;
        x[k] = in[k] ? (double)P[(size_t)i * 3 + 0] : 0.0;
        y[k] = in[k] ? (double)P[(size_t)i * 3 + 1] : 0.0;
        z[k] = in[k] ? (double)P[(size_t)i * 3 + 2] : 0.0;
    }
    const double* K = intr + (size_t)s * 6;
    const double fx = K[0], fy = K[1], cx = K[2], cy = K[3], u_max = K[4], v_max = K[5];
    for (int j = 0; j < nfr; ++j) {
        const double* M = w2c + (size_t)(S.f0 + fb + j) * 12;                 // wave-uniform: scalar registers
        const double m00 = M[0], m01 = M[1], m02 = M[2], m03 = M[3], m10 = M[4], m11 = M[5], m12 = M[6], m13 = M[7], m20 = M[8], m21 = M[9],
                     m22 = M[10], m23 = M[11];
#pragma unroll
        for (int k = 0; k < VIS_PPL; ++k) {
            const double X = __dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(x[k], m00), __dmul_rn(y[k], m01)), __dmul_rn(z[k], m02)), m03);
            const double Y = __dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(x[k], m10), __dmul_rn(y[k], m11)), __dmul_rn(z[k], m12)), m13);
            const double Z = __dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(x[k], m20), __dmul_rn(y[k], m21)), __dmul_rn(z[k], m22)), m23);
            const double r = (Z != 0.0) ? __ddiv_rn(1.0, Z) : 1.0;
            const double u = __dadd_rn(__dmul_rn(__dmul_rn(X, r), fx), cx);
            const double v = __dadd_rn(__dmul_rn(__dmul_rn(Y, r), fy), cy);
            const bool seen = in[k] && (Z > 0.0) && (u >= 0.0) && (u <= u_max) && (v >= 0.0) && (v <= v_max);      // all false on NaN
            const u64 word = __ballot(seen);
            if (lane == 0) sw[j][wave * VIS_PPL + k] = word;
        }
    }
    __syncthreads();
    const int j = tid / VIS_WORDS, w = tid % VIS_WORDS;
    const long long col = (long long)pt * VIS_WORDS + w;
    if (j < nfr && col < S.W) vis[S.v0 + (long long)(fb + j) * S.W + col] = sw[j][w];
}

// One workgroup per scan.  Frame f: cum[f] = vis[f] | (cum[f - 1] unless frame f - 1 closed a subscan); every lane re-reads only the words
// it wrote itself one frame earlier, so no ordering between lanes is needed on the matrix, only the block-wide sum of the popcounts.
__global__ __launch_bounds__(WALK_THREADS) void walk_kernel(const u64* vis, u64* cum, const int* __restrict__ pt_off, const int* __restrict__ fr_off,
                                                            const long long* __restrict__ vis_off, const int* __restrict__ max_pts, int n_scans,
                                                            int total_points, int total_frames, long long total_words, int* __restrict__ seg_end,
                                                            int* __restrict__ seg_count, int* __restrict__ frame_count, int* __restrict__ n_seg) {
    __shared__ int part[2][WALK_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int s = blockIdx.x;
    const VScan S = vis_scan(pt_off, fr_off, vis_off, n_scans, total_points, total_frames, total_words, s);
    if (!S.ok) return;
    if (S.n == 0 || S.nf == 0) {
        if (tid == 0) n_seg[s] = 0;
        return;
    }
    const int budget = max_pts[s];
    bool fresh = true;                                       // the running union is empty: at the start and after a closed subscan
    int k = 0;
    for (int f = 0; f < S.nf; ++f) {
        const u64* V = vis + S.v0 + (long long)f * S.W;
        u64* C = cum + S.v0 + (long long)f * S.W;
        int c = 0;
        for (long long w = tid; w < S.W; w += WALK_THREADS) {
            u64 v = V[w];
            if (!fresh) v |= (C - S.W)[w];
            C[w] = v;
            c += __popcll(v);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
        int* pp = part[f & 1];                               // two buffers: one barrier per frame is enough
        if (lane == 0) pp[wave] = c;
        __syncthreads();
        int tot = 0;
#pragma unroll
        for (int i = 0; i < WALK_THREADS / 64; ++i) tot += pp[i];
        fresh = tot >= budget;
        if (tid == 0) {
            frame_count[S.f0 + f] = tot;
            if (fresh) {
                seg_end[S.f0 + k] = f;
                seg_count[S.f0 + k] = tot;
            }
        }
        k += fresh ? 1 : 0;
    }
    if (tid == 0) n_seg[s] = k;
}

__global__ __launch_bounds__(OC_THREADS) void objcount_kernel(const u64* __restrict__ bits, const int* __restrict__ pt_off,
                                                              const int* __restrict__ fr_off, const long long* __restrict__ vis_off, int n_scans,
                                                              int total_points, int total_frames, long long total_words,
                                                              const int* __restrict__ rows, const int* __restrict__ slot, int n_slots, int p_tiles,
                                                              int* __restrict__ counts) {
    __shared__ int hist[VIS_LDS_SLOTS];
    const int tid = threadIdx.x;
    const int r = blockIdx.x / p_tiles, t = blockIdx.x % p_tiles;
    const int s = rows[2 * r], f = rows[2 * r + 1];
    const VScan S = vis_scan(pt_off, fr_off, vis_off, n_scans, total_points, total_frames, total_words, s);
    if (!S.ok || f < 0 || f >= S.nf) return;
    const long long pb = (long long)t * OC_TILE;
    if (pb >= S.n) return;
    const bool in_lds = n_slots <= VIS_LDS_SLOTS;
    int* out = counts + (size_t)r * n_slots;
    if (in_lds) {
        for (int i = tid; i < n_slots; i += OC_THREADS) hist[i] = 0;
        __syncthreads();
    }
    const u64* R = bits + S.v0 + (long long)f * S.W;
    const int* SL = slot + S.p0;
#pragma unroll 4
    for (int k = 0; k < OC_PPL; ++k) {
        const long long p = pb + k * OC_THREADS + tid;
        if (p >= S.n) break;
        if (!((R[p >> 6] >> (p & 63)) & 1ull)) continue;
        const int sl = SL[p];
        if (sl < 0 || sl >= n_slots) continue;               // a slot outside the table is not counted, never written
        if (in_lds)
            atomicAdd(&hist[sl], 1);
        else
            atomicAdd(&out[sl], 1);
    }
    if (in_lds) {
        __syncthreads();
        for (int i = tid; i < n_slots; i += OC_THREADS) {
            const int h = hist[i];
            if (h) atomicAdd(&out[i], h);
        }
    }
}

// The host copies of the offset arrays, when given: monotone, covering, and vis_off the prefix sum of F_t * ceil(N_t / 64).
int vis_check_host(const char* who, int n_scans, int total_points, int total_frames, long long total_words, const int32_t* pt_off_host,
                   const int32_t* fr_off_host, const int64_t* vis_off_host) {
    const SgaPrefix PT_OFF{"pt_off", "decreases", "scan", "total_points", nullptr, nullptr};
    const SgaPrefix FR_OFF{"fr_off", "decreases", "scan", "total_frames", nullptr, nullptr};
    if (int rc = sga_check_prefix(who, PT_OFF, pt_off_host, n_scans, total_points, SGA_ANY)) return rc;
    if (int rc = sga_check_prefix(who, FR_OFF, fr_off_host, n_scans, total_frames, SGA_ANY)) return rc;
    if (vis_off_host) {
        SGA_CHECK_ARG(vis_off_host[0] == 0, "%s: vis_off must start at 0", who);
        for (int i = 0; i < n_scans; ++i) {
            SGA_CHECK_ARG(vis_off_host[i + 1] >= vis_off_host[i], "%s: vis_off decreases at scan %d", who, i);
            if (pt_off_host && fr_off_host) {
                const long long W = ((long long)(pt_off_host[i + 1] - pt_off_host[i]) + 63) / 64;
                SGA_CHECK_ARG(vis_off_host[i + 1] - vis_off_host[i] == (long long)(fr_off_host[i + 1] - fr_off_host[i]) * W,
                              "%s: vis_off of scan %d is not frames x ceil(points / 64) words", who, i);
            }
        }
        SGA_CHECK_ARG(vis_off_host[n_scans] <= total_words, "%s: vis_off ends at %lld of %lld words", who, (long long)vis_off_host[n_scans],
                      total_words);
    }
    return SGA_OK;
}

}  // namespace

extern "C" int sga_subscan_lds_slots(void) { return VIS_LDS_SLOTS; }

extern "C" int sga_frame_visibility(const float* pts, const int32_t* pt_off, const double* w2c, const int32_t* fr_off, const double* intr,
                                    const int64_t* vis_off, int n_scans, int total_points, int total_frames, int64_t total_words, int max_points,
                                    int max_frames, const int32_t* pt_off_host, const int32_t* fr_off_host, const int64_t* vis_off_host,
                                    uint64_t* vis, void* stream) {
    SGA_CHECK_ARG(n_scans >= 0 && total_points >= 0 && total_frames >= 0 && total_words >= 0 && max_points >= 0 && max_frames >= 0,
                  "sga_frame_visibility: negative count (n_scans %d, total_points %d, total_frames %d, total_words %lld, max_points %d, max_frames %d)",
                  n_scans, total_points, total_frames, (long long)total_words, max_points, max_frames);
    SGA_CHECK_ARG(max_points <= total_points && max_frames <= total_frames, "sga_frame_visibility: max_points %d / max_frames %d exceed the totals %d / %d",
                  max_points, max_frames, total_points, total_frames);
    if (n_scans == 0 || max_points == 0 || max_frames == 0 || total_words == 0) return SGA_OK;               // nothing to write
    SGA_CHECK_ARG(pts && pt_off && w2c && fr_off && intr && vis_off && vis, "sga_frame_visibility: null pointer");
    SGA_CHECK_ARG(sga_aligned(8, w2c, intr, vis_off, vis) && sga_aligned(4, pts, pt_off, fr_off),
                  "sga_frame_visibility: misaligned pointer (64-bit arrays need 8 bytes, 32-bit arrays 4)");
    if (int rc = vis_check_host("sga_frame_visibility", n_scans, total_points, total_frames, total_words, pt_off_host, fr_off_host, vis_off_host)) return rc;
    if (pt_off_host && fr_off_host)
        for (int i = 0; i < n_scans; ++i)
            SGA_CHECK_ARG(pt_off_host[i + 1] - pt_off_host[i] <= max_points && fr_off_host[i + 1] - fr_off_host[i] <= max_frames,
                          "sga_frame_visibility: scan %d is larger than max_points %d / max_frames %d", i, max_points, max_frames);
    const long p_tiles = ((long)max_points + VIS_PTILE - 1) / VIS_PTILE, f_groups = ((long)max_frames + VIS_FG - 1) / VIS_FG;
    if (int rc = sga_check_grid("sga_frame_visibility", p_tiles, f_groups, n_scans, "split the scan list")) return rc;
    hipLaunchKernelGGL(vis_kernel, dim3((unsigned)(p_tiles * f_groups * n_scans)), dim3(VIS_THREADS), 0, static_cast<hipStream_t>(stream), pts, pt_off,
                       w2c, fr_off, intr, reinterpret_cast<const long long*>(vis_off), n_scans, total_points, total_frames, (long long)total_words,
                       (int)p_tiles, (int)f_groups, reinterpret_cast<u64*>(vis));
    SGA_CHECK_LAUNCH("sga_frame_visibility");
    return SGA_OK;
}

extern "C" int sga_subscan_walk(const uint64_t* vis, uint64_t* cum, const int32_t* pt_off, const int32_t* fr_off, const int64_t* vis_off,
                                const int32_t* max_pts, int n_scans, int total_points, int total_frames, int64_t total_words,
                                const int32_t* pt_off_host, const int32_t* fr_off_host, const int64_t* vis_off_host, int32_t* seg_end,
                                int32_t* seg_count, int32_t* frame_count, int32_t* n_seg, void* stream) {
    SGA_CHECK_ARG(n_scans >= 0 && total_points >= 0 && total_frames >= 0 && total_words >= 0,
                  "sga_subscan_walk: negative count (n_scans %d, total_points %d, total_frames %d, total_words %lld)", n_scans, total_points,
                  total_frames, (long long)total_words);
    if (n_scans == 0) return SGA_OK;
    SGA_CHECK_ARG(pt_off && fr_off && vis_off && max_pts && n_seg, "sga_subscan_walk: null pointer");
    SGA_CHECK_ARG((vis && cum) || total_words == 0, "sga_subscan_walk: null bit matrix");
    SGA_CHECK_ARG((seg_end && seg_count && frame_count) || total_frames == 0, "sga_subscan_walk: null output");
    SGA_CHECK_ARG(sga_aligned(8, vis, cum, vis_off) && sga_aligned(4, pt_off, fr_off, max_pts, seg_end, seg_count, frame_count, n_seg),
                  "sga_subscan_walk: misaligned pointer (64-bit arrays need 8 bytes, 32-bit arrays 4)");
    if (int rc = vis_check_host("sga_subscan_walk", n_scans, total_points, total_frames, total_words, pt_off_host, fr_off_host, vis_off_host)) return rc;
    hipLaunchKernelGGL(walk_kernel, dim3((unsigned)n_scans), dim3(WALK_THREADS), 0, static_cast<hipStream_t>(stream), reinterpret_cast<const u64*>(vis),
                       reinterpret_cast<u64*>(cum), pt_off, fr_off, reinterpret_cast<const long long*>(vis_off), max_pts, n_scans, total_points,
                       total_frames, (long long)total_words, seg_end, seg_count, frame_count, n_seg);
    SGA_CHECK_LAUNCH("sga_subscan_walk");
    return SGA_OK;
}

extern "C" int sga_subscan_object_counts(const uint64_t* bits, const int32_t* pt_off, const int32_t* fr_off, const int64_t* vis_off, int n_scans,
                                         int total_points, int total_frames, int64_t total_words, int max_points, const int32_t* rows, int n_rows,
                                         const int32_t* slot, int n_slots, const int32_t* pt_off_host, const int32_t* fr_off_host,
                                         const int64_t* vis_off_host, const int32_t* rows_host, int32_t* counts, void* stream) {
    SGA_CHECK_ARG(n_scans >= 0 && total_points >= 0 && total_frames >= 0 && total_words >= 0 && max_points >= 0 && n_rows >= 0 && n_slots >= 0,
                  "sga_subscan_object_counts: negative count (n_scans %d, total_points %d, total_frames %d, total_words %lld, max_points %d, n_rows %d, "
                  "n_slots %d)", n_scans, total_points, total_frames, (long long)total_words, max_points, n_rows, n_slots);
    SGA_CHECK_ARG(max_points <= total_points, "sga_subscan_object_counts: max_points %d exceeds total_points %d", max_points, total_points);
    if (n_rows == 0 || n_slots == 0) return SGA_OK;                                                          // nothing to write
    const bool empty = max_points == 0 || total_words == 0;                                                  // empty scans only: all counts are 0
    SGA_CHECK_ARG(counts && (empty || (bits && pt_off && fr_off && vis_off && rows && slot)), "sga_subscan_object_counts: null pointer");
    SGA_CHECK_ARG((long)n_rows * n_slots < (1L << 31), "sga_subscan_object_counts: %d rows x %d slots exceed 2^31 counters", n_rows, n_slots);
    SGA_CHECK_ARG(sga_aligned(8, bits, vis_off) && sga_aligned(4, pt_off, fr_off, rows, slot, counts),
                  "sga_subscan_object_counts: misaligned pointer (64-bit arrays need 8 bytes, 32-bit arrays 4)");
    if (int rc = vis_check_host("sga_subscan_object_counts", n_scans, total_points, total_frames, total_words, pt_off_host, fr_off_host, vis_off_host))
        return rc;
    if (rows_host)
        for (int r = 0; r < n_rows; ++r) {
            const int s = rows_host[2 * r], f = rows_host[2 * r + 1];
            SGA_CHECK_ARG(s >= 0 && s < n_scans, "sga_subscan_object_counts: row %d names scan %d of %d", r, s, n_scans);
            if (fr_off_host) SGA_CHECK_ARG(f >= 0 && f < fr_off_host[s + 1] - fr_off_host[s], "sga_subscan_object_counts: row %d names frame %d of %d", r, f,
                                           fr_off_host[s + 1] - fr_off_host[s]);
            if (pt_off_host) SGA_CHECK_ARG(pt_off_host[s + 1] - pt_off_host[s] <= max_points, "sga_subscan_object_counts: scan %d is larger than max_points %d",
                                           s, max_points);
        }
    hipStream_t st = static_cast<hipStream_t>(stream);
    const long p_tiles = ((long)max_points + OC_TILE - 1) / OC_TILE;
    if (int rc = sga_check_grid("sga_subscan_object_counts", p_tiles, 1, n_rows, "split the row list")) return rc;
    if (int rc = sga_zero("sga_subscan_object_counts", counts, (size_t)n_rows * n_slots * sizeof(int32_t), st)) return rc;
    if (empty) return SGA_OK;
    hipLaunchKernelGGL(objcount_kernel, dim3((unsigned)(p_tiles * n_rows)), dim3(OC_THREADS), 0, st, reinterpret_cast<const u64*>(bits), pt_off, fr_off,
                       reinterpret_cast<const long long*>(vis_off), n_scans, total_points, total_frames, (long long)total_words, rows, slot, n_slots,
                       (int)p_tiles, counts);
    SGA_CHECK_LAUNCH("sga_subscan_object_counts");
    return SGA_OK;
}
