// The pair-job contract of the nearest-neighbour searches (nnsearch.hip, featnn.hip) on top of the packed-segment contract: a job is a
// (query set, support set) pair of ids into one packed array, job p writes its nq results at out_off[p], and a support longer than `chunk`
// is split over workgroups whose partials are folded in ascending chunk order with a strict <.  The device half re-derives every range
// from the device arrays and does nothing on a bad one; the host half refuses a bad job list before anything is launched.  sga_segment is
// the lookup under it: sga_cloud calls it; sga_pair_job, sga_cloud_pair and sga_hyp_job write it out (the call changes their kernels' code
// objects).  The hypothesis-job lookup of ransac.hip / ransac_geo.hip and the cloud lookups of fpfh.hip / voxel.hip stand here too, once.
#pragma once
#include "packed.h"

struct SgaSegment { int o0, n; bool ok; };
struct SgaPairJob { int q0, nq, s0, ns, oo; bool ok; };
struct SgaCloudPair { int q0, nq, s0, ns, sc; bool ok; };
struct SgaHypJob { int o0, n, h0, nh; bool ok; };
struct SgaCloud { int o0, n, c; bool ok; };

// Segment i of a packed array, [off[i], off[i + 1]), range-checked against `total`: a bad offset gives {0, 0, false}.
__device__ __forceinline__ SgaSegment sga_segment(const int* __restrict__ off, int total, int i) {
    const int o0 = off[i], o1 = off[i + 1];
    if (o0 < 0 || o1 < o0 || o1 > total) return SgaSegment{0, 0, false};
    return SgaSegment{o0, o1 - o0, true};
}

// Everything a workgroup needs to know about job `job`, read from the device arrays and range-checked -- the job id, the two set ids, both
// segments and the output range: a bad id or offset makes the workgroup do nothing instead of reading or writing out of bounds.
__device__ __forceinline__ SgaPairJob sga_pair_job(const int* __restrict__ off, int n_sets, int total_rows, const int* __restrict__ pairs,
                                                   int n_pairs, const int* __restrict__ out_off, int total_queries, int job) {
    const SgaPairJob none{0, 0, 0, 0, 0, false};
    if (job < 0 || job >= n_pairs) return none;
    const int qc = pairs[2 * job], sc = pairs[2 * job + 1];
    if (qc < 0 || qc >= n_sets || sc < 0 || sc >= n_sets) return none;
    const int q0 = off[qc], q1 = off[qc + 1], s0 = off[sc], s1 = off[sc + 1], oo = out_off[job];
    if (q0 < 0 || q1 < q0 || q1 > total_rows || s0 < 0 || s1 < s0 || s1 > total_rows) return none;
    if (oo < 0 || oo > total_queries || q1 - q0 > total_queries - oo) return none;
    return SgaPairJob{q0, q1 - q0, s0, s1 - s0, oo, true};
}

// sga_pair_job without the output range: the job id, the two cloud ids and both segments, read from the device arrays and range-checked.
__device__ __forceinline__ SgaCloudPair sga_cloud_pair(const int* __restrict__ off, int n_clouds, int total_points, const int* __restrict__ pairs,
                                                       int n_pairs, int job) {
    const SgaCloudPair none{0, 0, 0, 0, 0, false};
    if (job < 0 || job >= n_pairs) return none;
    const int qc = pairs[2 * job], sc = pairs[2 * job + 1];
    if (qc < 0 || qc >= n_clouds || sc < 0 || sc >= n_clouds) return none;
    const int q0 = off[qc], q1 = off[qc + 1], s0 = off[sc], s1 = off[sc + 1];
    if (q0 < 0 || q1 < q0 || q1 > total_points || s0 < 0 || s1 < s0 || s1 > total_points) return none;
    return SgaCloudPair{q0, q1 - q0, s0, s1 - s0, sc, true};
}

// Rows and hypotheses of RANSAC job `job`, range-checked (two sga_segment lookups, written out): a bad offset makes the caller do nothing.
__device__ __forceinline__ SgaHypJob sga_hyp_job(const int* __restrict__ off, int total_rows, const int* __restrict__ hoff, int total_hyp, int job) {
    const int o0 = off[job], o1 = off[job + 1], h0 = hoff[job], h1 = hoff[job + 1];
    if (o0 < 0 || o1 < o0 || o1 > total_rows || h0 < 0 || h1 < h0 || h1 > total_hyp) return SgaHypJob{0, 0, 0, 0, false};
    return SgaHypJob{o0, o1 - o0, h0, h1 - h0, true};
}

// Cloud c of the packed array, range-checked.
__device__ __forceinline__ SgaCloud sga_cloud(const int* __restrict__ off, int total_points, int c) {
    const SgaSegment s = sga_segment(off, total_points, c);
    return SgaCloud{s.o0, s.n, c, s.ok};
}

// The cloud that holds packed row i: the LAST c with offsets[c] <= i (empty clouds repeat an offset), re-checked.
__device__ __forceinline__ SgaCloud sga_cloud_of_point(const int* __restrict__ off, int n_clouds, int total_points, int i) {
    int lo = 0, hi = n_clouds - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (off[mid] <= i) lo = mid; else hi = mid - 1;
    }
    const SgaCloud C = sga_cloud(off, total_points, lo);
    if (!C.ok || i < C.o0 || i - C.o0 >= C.n) return SgaCloud{0, 0, lo, false};
    return C;
}

// Passes over a support of ns rows in chunks of `chunk` (>= 1).  An empty support still takes one pass: the one that writes "no neighbour".
__host__ __device__ __forceinline__ int sga_chunks(int ns, int chunk) { return ns <= chunk ? 1 : (int)(((long long)ns + chunk - 1) / chunk); }

// The job list's host copy (null: skipped): every pair names two of the n_sets `unit`s ("cloud", "set"), none longer than the grid is sized for.
static inline int sga_check_pairs(const char* who, const char* unit, const int32_t* pairs_host, int n_pairs, const int32_t* offsets_host, int n_sets,
                                  int max_queries, int max_support) {
    if (!pairs_host) return SGA_OK;
    for (int p = 0; p < n_pairs; ++p) {
        const int qc = pairs_host[2 * p], sc = pairs_host[2 * p + 1];
        SGA_CHECK_ARG(qc >= 0 && qc < n_sets && sc >= 0 && sc < n_sets, "%s: pair %d names %s (%d, %d) of %d", who, p, unit, qc, sc, n_sets);
        SGA_CHECK_ARG(!offsets_host || (offsets_host[qc + 1] - offsets_host[qc] <= max_queries && offsets_host[sc + 1] - offsets_host[sc] <= max_support),
                      "%s: pair %d is larger than max_queries %d / max_support %d", who, p, max_queries, max_support);
    }
    return SGA_OK;
}

// The two argument checks every chunked search shares.
static inline int sga_check_chunked(const char* who, int chunk, int max_queries, int total_queries) {
    SGA_CHECK_ARG(chunk >= 1, "%s: chunk must be >= 1 (got %d)", who, chunk);
    SGA_CHECK_ARG(max_queries <= total_queries, "%s: max_queries %d exceeds total_queries %d", who, max_queries, total_queries);
    return SGA_OK;
}

// A call that needs `need` > 0 bytes of workspace was given at least that many.
static inline int sga_check_workspace(const char* who, size_t need, const void* workspace, size_t workspace_bytes) {
    if (need > 0 && (!workspace || workspace_bytes < need)) {
        sga_set_error("%s: workspace of %zu bytes needed, %zu given", who, need, workspace ? workspace_bytes : (size_t)0);
        return SGA_ERR_WORKSPACE;
    }
    return SGA_OK;
}
