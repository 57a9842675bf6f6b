// Batched scene-graph records: per-object point counts, the stable split of a scan into its objects, the completion of a listed edge set
// to every ordered pair with its (misaligned, see below) relation bag-of-words, and a plain (row, col) -> count scatter.
//
// Replaces the host loops of preprocessing/scan3r/preprocess.py: the per-object `np.where(objectId == id)` (:86-87), the `none`-edge
// supplement `for i: for j: [i, j] in pairs` (:176-182) and the bag-of-words passes (:280-361).  Integers only: every sum in this file is
// an integer atomic (order-independent) or a prefix sum taken in index order, so every output is a pure function of the input.
//
// Scans are packed back to back: slot [sum N] int32 is each point's dense object slot within its scan (-1 or any value outside the scan's
// slot range: the point belongs to no object), pt_off [S + 1] / slot_off [S + 1] the point and slot ranges.
//
// object_counts_kernel: one lane per point, a workgroup-private LDS histogram flushed with integer atomics (global integer atomics above
// SG_LDS_SLOTS slots per scan), as objcount_kernel of visibility.hip does for one bit row.
//
// The partition is three launches over tiles of SG_TILE points.  (1) tile_hist_kernel: the histogram of every tile, one row of max_slots
// counters per (scan, tile) in the workspace.  (2) tile_scan_kernel: one lane per (scan, slot) turns its column into the exclusive prefix
// over tiles, in tile order.  (3) tile_place_kernel: one wave per tile walks the tile in 64-point chunks in point order; inside a chunk the
// rank of a point among the points of its slot is the popcount of a __ballot below its lane, and a per-slot running base in LDS carries the
// count from chunk to chunk.  Destination = dest_off[slot] + tile prefix + running base + rank: ascending point order, never the arrival
// order of an atomic.
//
// graph_complete_kernel: one workgroup per graph.  The adjacency bit matrix (N rows of ceil(N / 32) words) lives in LDS next to one counter
// per row; listed pairs set bits with LDS atomicOr (order-independent), every row counts its missing entries (popcount), wave 0 takes the
// exclusive prefix over rows, and one wave per row writes the row's missing j ascending.  bow[edges[idx][0], rel(idx)] += 1 with rel(idx) the
// idx-th entry of the TRIPLES list (listed triples, then `none`): the reference indexes the triples with the edge index
// (preprocess.py:303-306), and the triples list is longer than the pair list whenever a pair is listed with two relations.
// Every kernel re-derives its ranges from the device offset arrays and does nothing on a bad one.
#include "packed.h"

#include <algorithm>
#include <vector>

namespace {

typedef unsigned long long u64;

constexpr int SG_THREADS = 256;
constexpr int SG_TILE = 2048;                                // points per partition tile (and per workgroup of the count kernel)
constexpr int SG_LDS_SLOTS = 4096;                           // slots per scan served from LDS (16 KiB); the partition refuses more
constexpr int GC_THREADS = 256;
constexpr int GC_LDS_WORDS = (64 * 1024 - 256) / 4;          // the static LDS limit of a workgroup, less the scan's scratch

constexpr int gc_row_words(int n) { return (n + 31) / 32; }
constexpr int gc_max_nodes() {
    int n = 0;
    while ((long)(n + 1) * gc_row_words(n + 1) + (n + 1) <= GC_LDS_WORDS) ++n;
    return n;
}
constexpr int GC_MAX_NODES = gc_max_nodes();                 // 704: 704 x 22 words of bits + 704 row counters

struct SScan { int p0, n, k0, nk; bool ok; };

__device__ __forceinline__ SScan sg_scan(const int* __restrict__ pt_off, const int* __restrict__ slot_off, int n_scans, int total_points,
                                         int total_slots, int s) {
    SScan S{0, 0, 0, 0, false};
    if (s < 0 || s >= n_scans) return S;
    const int p0 = pt_off[s], p1 = pt_off[s + 1], k0 = slot_off[s], k1 = slot_off[s + 1];
    if (p0 < 0 || p1 < p0 || p1 > total_points || k0 < 0 || k1 < k0 || k1 > total_slots) return S;
    return SScan{p0, p1 - p0, k0, k1 - k0, true};
}

__global__ __launch_bounds__(SG_THREADS) void object_counts_kernel(const int* __restrict__ slot, const int* __restrict__ pt_off,
                                                                   const int* __restrict__ slot_off, int n_scans, int total_points,
                                                                   int total_slots, int p_tiles, int* __restrict__ counts) {
    __shared__ int hist[SG_LDS_SLOTS];
    const int tid = threadIdx.x;
    const int s = blockIdx.x / p_tiles, t = blockIdx.x % p_tiles;
    const SScan S = sg_scan(pt_off, slot_off, n_scans, total_points, total_slots, s);
    if (!S.ok || S.nk == 0) return;
    const long long pb = (long long)t * SG_TILE;
    if (pb >= S.n) return;
    const bool in_lds = S.nk <= SG_LDS_SLOTS;
    int* out = counts + S.k0;
    if (in_lds) {
        for (int i = tid; i < S.nk; i += SG_THREADS) hist[i] = 0;
        __syncthreads();
    }
    const int* SL = slot + S.p0;
    for (int k = 0; k < SG_TILE / SG_THREADS; ++k) {
        const long long p = pb + k * SG_THREADS + tid;
        if (p >= S.n) break;
        const int sl = SL[p];
        if (sl < 0 || sl >= S.nk) continue;                  // a slot outside the scan's table is not counted, never written
        if (in_lds)
            atomicAdd(&hist[sl], 1);
        else
            atomicAdd(&out[sl], 1);
    }
    if (in_lds) {
        __syncthreads();
        for (int i = tid; i < S.nk; i += SG_THREADS) {
            const int h = hist[i];
            if (h) atomicAdd(&out[i], h);
        }
    }
}

// ---- partition -----------------------------------------------------------------------------------------------------------------------
// Workspace: int32 [n_scans][p_tiles][max_slots]; row (s, t) holds tile t's histogram after pass 1, its exclusive prefix over tiles after pass 2.
__global__ __launch_bounds__(SG_THREADS) void tile_hist_kernel(const int* __restrict__ slot, const int* __restrict__ pt_off,
                                                               const int* __restrict__ slot_off, int n_scans, int total_points, int total_slots,
                                                               int p_tiles, int max_slots, int* __restrict__ ws) {
    __shared__ int hist[SG_LDS_SLOTS];
    const int tid = threadIdx.x;
    const int s = blockIdx.x / p_tiles, t = blockIdx.x % p_tiles;
    const SScan S = sg_scan(pt_off, slot_off, n_scans, total_points, total_slots, s);
    if (!S.ok || S.nk == 0 || S.nk > max_slots || S.nk > SG_LDS_SLOTS) return;
    const long long pb = (long long)t * SG_TILE;
    if (pb >= S.n) return;
    for (int i = tid; i < S.nk; i += SG_THREADS) hist[i] = 0;
    __syncthreads();
    const int* SL = slot + S.p0;
    for (int k = 0; k < SG_TILE / SG_THREADS; ++k) {
        const long long p = pb + k * SG_THREADS + tid;
        if (p >= S.n) break;
        const int sl = SL[p];
        if (sl >= 0 && sl < S.nk) atomicAdd(&hist[sl], 1);
    }
    __syncthreads();
    int* row = ws + ((size_t)s * p_tiles + t) * max_slots;
    for (int i = tid; i < S.nk; i += SG_THREADS) row[i] = hist[i];
}

__global__ __launch_bounds__(SG_THREADS) void tile_scan_kernel(const int* __restrict__ pt_off, const int* __restrict__ slot_off, int n_scans,
                                                               int total_points, int total_slots, int p_tiles, int max_slots,
                                                               int* __restrict__ ws) {
    const long long id = (long long)blockIdx.x * SG_THREADS + threadIdx.x;
    const int s = (int)(id / max_slots), k = (int)(id % max_slots);
    const SScan S = sg_scan(pt_off, slot_off, n_scans, total_points, total_slots, s);
    if (!S.ok || k >= S.nk || S.nk > max_slots) return;
    const int tiles = min((int)(((long long)S.n + SG_TILE - 1) / SG_TILE), p_tiles);
    int* col = ws + (size_t)s * p_tiles * max_slots + k;
    int acc = 0;
    for (int t = 0; t < tiles; ++t) {
        const int v = col[(size_t)t * max_slots];
        col[(size_t)t * max_slots] = acc;
        acc += v;
    }
}

__global__ __launch_bounds__(64) void tile_place_kernel(const float* __restrict__ pts, const int* __restrict__ slot, const int* __restrict__ pt_off,
                                                        const int* __restrict__ slot_off, const int* __restrict__ dest_off, int n_scans,
                                                        int total_points, int total_slots, int p_tiles, int max_slots, const int* __restrict__ ws,
                                                        int n_kept, int* __restrict__ perm, float* __restrict__ pts_out) {
    __shared__ int run[SG_LDS_SLOTS];                        // destination of the slot's next point: dest_off + tile prefix + points placed so far
    const int lane = threadIdx.x;
    const int s = blockIdx.x / p_tiles, t = blockIdx.x % p_tiles;
    const SScan S = sg_scan(pt_off, slot_off, n_scans, total_points, total_slots, s);
    if (!S.ok || S.nk == 0 || S.nk > max_slots || S.nk > SG_LDS_SLOTS) return;
    const long long pb = (long long)t * SG_TILE;
    if (pb >= S.n) return;
    const int* row = ws + ((size_t)s * p_tiles + t) * max_slots;
    for (int i = lane; i < S.nk; i += 64) {
        const int d = dest_off[S.k0 + i];
        run[i] = d < 0 ? -1 : d + row[i];
    }
    __syncthreads();
    const int* SL = slot + S.p0;
    const float* P = pts + (size_t)S.p0 * 3;
    const u64 below = (1ull << lane) - 1ull;
    for (int c = 0; c < SG_TILE / 64; ++c) {
        const long long p = pb + c * 64 + lane;
        if (pb + c * 64 >= S.n) break;                       // wave-uniform
        int k = p < S.n ? SL[p] : -1;
        bool keep = k >= 0 && k < S.nk;
        if (keep) keep = run[k] >= 0;                        // a dropped slot never changes its -1
        u64 todo = __ballot(keep);
        while (todo) {                                       // one round per distinct slot of the chunk
            const int leader = __ffsll((long long)todo) - 1;
            const int kk = __shfl(k, leader, 64);
            const bool mine = keep && k == kk;
            const u64 m = __ballot(mine);
            const int base = run[kk];                        // every lane reads before the leader writes: one wave, program order
            if (mine) {
                const long long pos = (long long)base + __popcll(m & below);
                if (pos < n_kept) {
                    perm[pos] = (int)p;
                    pts_out[pos * 3 + 0] = P[p * 3 + 0];
                    pts_out[pos * 3 + 1] = P[p * 3 + 1];
                    pts_out[pos * 3 + 2] = P[p * 3 + 2];
                }
            }
            if (lane == leader) run[kk] = base + __popcll(m);
            todo &= ~m;
        }
    }
}

// ---- edge completion -------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned gc_missing(const unsigned* adj, int N, int W, int i, int w) {
    unsigned m = ~adj[i * W + w];
    if (w == W - 1 && (N & 31)) m &= (1u << (N & 31)) - 1u;
    if (w == (i >> 5)) m &= ~(1u << (i & 31));
    return m;
}

__global__ __launch_bounds__(GC_THREADS) void graph_complete_kernel(const int* __restrict__ node_off, const int* __restrict__ pair_off,
                                                                    const int* __restrict__ trip_off, const int* __restrict__ edge_off,
                                                                    int n_graphs, int total_nodes, int total_pairs, int total_trips,
                                                                    int total_edges, const int* __restrict__ pairs, const int* __restrict__ rels,
                                                                    int none_id, int V, long long* __restrict__ edges, int* __restrict__ n_edges,
                                                                    int* __restrict__ bow) {
    __shared__ unsigned lds[GC_LDS_WORDS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int g = blockIdx.x;
    if (g >= n_graphs) return;
    const int b0 = node_off[g], N = node_off[g + 1] - b0, q0 = pair_off[g], P = pair_off[g + 1] - q0, t0 = trip_off[g],
              Tr = trip_off[g + 1] - t0, e0 = edge_off[g], cap = edge_off[g + 1] - e0;
    if (b0 < 0 || N < 0 || N > GC_MAX_NODES || b0 + N > total_nodes || q0 < 0 || P < 0 || q0 + P > total_pairs || t0 < 0 || Tr < P ||
        t0 + Tr > total_trips || e0 < 0 || cap < 0 || e0 + cap > total_edges || (long long)P + (long long)N * (N - 1) > cap || none_id < 0 ||
        none_id >= V)
        return;
    const int W = gc_row_words(N);
    unsigned* adj = lds;
    int* rowoff = reinterpret_cast<int*>(lds + N * W);
    for (int i = tid; i < N * W; i += GC_THREADS) adj[i] = 0u;
    __syncthreads();
    for (int p = tid; p < P; p += GC_THREADS) {
        const int i = pairs[2 * (size_t)(q0 + p)], j = pairs[2 * (size_t)(q0 + p) + 1];
        edges[2 * (size_t)(e0 + p)] = i;
        edges[2 * (size_t)(e0 + p) + 1] = j;
        const bool ok_i = i >= 0 && i < N;
        if (ok_i && j >= 0 && j < N && i != j) atomicOr(&adj[i * W + (j >> 5)], 1u << (j & 31));
        const int r = rels[t0 + p];
        if (ok_i && r >= 0 && r < V) atomicAdd(&bow[(size_t)(b0 + i) * V + r], 1);
    }
    __syncthreads();
    for (int i = tid; i < N; i += GC_THREADS) {
        int c = 0;
        for (int w = 0; w < W; ++w) c += __popc(gc_missing(adj, N, W, i, w));
        rowoff[i] = c;
    }
    __syncthreads();
    if (wave == 0) {                                         // exclusive prefix over rows, in row order
        int carry = 0;
        for (int base = 0; base < N; base += 64) {
            const int i = base + lane;
            const int v = i < N ? rowoff[i] : 0;
            const int incl = wave_incl_scan(v, lane);
            if (i < N) rowoff[i] = carry + incl - v;
            carry += __shfl(incl, 63, 64);
        }
        if (lane == 0) n_edges[g] = P + carry;
    }
    __syncthreads();
    for (int i = wave; i < N; i += GC_THREADS / 64) {        // one wave per row: the row's missing j, ascending
        int pos = P + rowoff[i];
        int n_none = 0;
        for (int wb = 0; wb < W; wb += 64) {
            const int w = wb + lane;
            unsigned m = w < W ? gc_missing(adj, N, W, i, w) : 0u;
            const int c = __popc(m);
            const int incl = wave_incl_scan(c, lane);
            int idx = pos + incl - c;
            while (m) {
                const int j = w * 32 + __ffs((int)m) - 1;
                m &= m - 1u;
                edges[2 * (size_t)(e0 + idx)] = i;
                edges[2 * (size_t)(e0 + idx) + 1] = j;
                if (idx < Tr) {                              // the edge index still points into the LISTED triples: their relation, not `none`
                    const int r = rels[t0 + idx];
                    if (r >= 0 && r < V) atomicAdd(&bow[(size_t)(b0 + i) * V + r], 1);
                } else {
                    ++n_none;
                }
                ++idx;
            }
            pos += __shfl(incl, 63, 64);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) n_none += __shfl_xor(n_none, o, 64);
        if (lane == 0 && n_none) atomicAdd(&bow[(size_t)(b0 + i) * V + none_id], n_none);
    }
}

__global__ __launch_bounds__(SG_THREADS) void bow_counts_kernel(const int* __restrict__ rows, const int* __restrict__ cols, int n, int T, int V,
                                                                int* __restrict__ out) {
    const long long i = (long long)blockIdx.x * SG_THREADS + threadIdx.x;
    if (i >= n) return;
    const int r = rows[i], c = cols[i];
    if (r < 0 || r >= T || c < 0 || c >= V) return;          // never written; the host check refuses such input
    atomicAdd(&out[(size_t)r * V + c], 1);
}

// A host copy sga_graph_complete cannot do without: it is where the totals come from.
int gc_offsets(const char* name, const int32_t* off, int n, long long* total) {
    SGA_CHECK_ARG(off != nullptr, "sga_graph_complete: %s (host copy) is null", name);
    *total = off[n];
    return sga_check_prefix("sga_graph_complete", SgaPrefix{name, "decreases", "", nullptr, nullptr, nullptr}, off, n, SGA_ANY, SGA_ANY);
}

const SgaPrefix PT_OFF{"pt_off", "decreases", "scan", "total_points", nullptr, nullptr};
const SgaPrefix SLOT_OFF{"slot_off", "decreases", "scan", "total_slots", nullptr, nullptr};

}  // namespace

extern "C" int sga_scenegraph_lds_slots(void) { return SG_LDS_SLOTS; }
extern "C" int sga_scenegraph_tile(void) { return SG_TILE; }
extern "C" int sga_graph_max_nodes(void) { return GC_MAX_NODES; }

extern "C" int sga_object_counts(const int32_t* slot, const int32_t* pt_off, const int32_t* slot_off, int n_scans, int total_points,
                                 int total_slots, int max_points, const int32_t* pt_off_host, const int32_t* slot_off_host, int32_t* counts,
                                 void* stream) {
    SGA_CHECK_ARG(n_scans >= 0 && total_points >= 0 && total_slots >= 0 && max_points >= 0,
                  "sga_object_counts: negative count (n_scans %d, total_points %d, total_slots %d, max_points %d)", n_scans, total_points,
                  total_slots, max_points);
    SGA_CHECK_ARG(max_points <= total_points, "sga_object_counts: max_points %d exceeds total_points %d", max_points, total_points);
    if (n_scans == 0 || total_slots == 0) return SGA_OK;                                                     // nothing to write
    SGA_CHECK_ARG(counts && (max_points == 0 || (slot && pt_off && slot_off)), "sga_object_counts: null pointer");
    SGA_CHECK_ARG(sga_aligned(4, slot, pt_off, slot_off, counts),
                  "sga_object_counts: misaligned pointer (32-bit arrays need 4 bytes)");
    if (int rc = sga_check_prefix("sga_object_counts", PT_OFF, pt_off_host, n_scans, total_points, SGA_ANY)) return rc;
    if (pt_off_host)
        for (int i = 0; i < n_scans; ++i)
            SGA_CHECK_ARG(pt_off_host[i + 1] - pt_off_host[i] <= max_points, "sga_object_counts: scan %d is larger than max_points %d", i, max_points);
    if (int rc = sga_check_prefix("sga_object_counts", SLOT_OFF, slot_off_host, n_scans, total_slots, SGA_ANY)) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (int rc = sga_zero("sga_object_counts", counts, (size_t)total_slots * sizeof(int32_t), st)) return rc;
    if (max_points == 0) return SGA_OK;
    const long p_tiles = ((long)max_points + SG_TILE - 1) / SG_TILE;
    if (int rc = sga_check_grid("sga_object_counts", p_tiles, 1, n_scans, "split the scan list")) return rc;
    hipLaunchKernelGGL(object_counts_kernel, dim3((unsigned)(p_tiles * n_scans)), dim3(SG_THREADS), 0, st, slot, pt_off, slot_off, n_scans,
                       total_points, total_slots, (int)p_tiles, counts);
    SGA_CHECK_LAUNCH("sga_object_counts");
    return SGA_OK;
}

extern "C" size_t sga_object_partition_ws_bytes(int n_scans, int max_points, int max_slots) {
    if (n_scans <= 0 || max_points <= 0 || max_slots <= 0) return 0;
    const size_t p_tiles = ((size_t)max_points + SG_TILE - 1) / SG_TILE;
    return (size_t)n_scans * p_tiles * (size_t)max_slots * sizeof(int32_t);
}

extern "C" int sga_object_partition(const float* pts, const int32_t* slot, const int32_t* pt_off, const int32_t* slot_off, const int32_t* dest_off,
                                    int n_scans, int total_points, int total_slots, int max_points, int max_slots, int n_kept_points,
                                    const int32_t* pt_off_host, const int32_t* slot_off_host, const int32_t* dest_off_host,
                                    const int32_t* counts_host, int32_t* perm, float* pts_out, void* ws, size_t ws_bytes, void* stream) {
    SGA_CHECK_ARG(n_scans >= 0 && total_points >= 0 && total_slots >= 0 && max_points >= 0 && max_slots >= 0 && n_kept_points >= 0,
                  "sga_object_partition: negative count (n_scans %d, total_points %d, total_slots %d, max_points %d, max_slots %d, n_kept_points %d)",
                  n_scans, total_points, total_slots, max_points, max_slots, n_kept_points);
    SGA_CHECK_ARG(max_points <= total_points && max_slots <= total_slots && n_kept_points <= total_points,
                  "sga_object_partition: max_points %d / max_slots %d / n_kept_points %d exceed the totals %d / %d", max_points, max_slots,
                  n_kept_points, total_points, total_slots);
    SGA_CHECK_ARG(max_slots <= SG_LDS_SLOTS, "sga_object_partition: %d slots in one scan, at most %d are supported", max_slots, SG_LDS_SLOTS);
    SGA_CHECK_ARG(pt_off_host && slot_off_host && dest_off_host && counts_host, "sga_object_partition: the host copies of the offsets are required");
    if (int rc = sga_prefix_ends("sga_object_partition", PT_OFF, pt_off_host, n_scans, total_points)) return rc;
    if (int rc = sga_prefix_ends("sga_object_partition", SLOT_OFF, slot_off_host, n_scans, total_slots)) return rc;
    for (int i = 0; i < n_scans; ++i) {
        if (int rc = sga_prefix_step("sga_object_partition", PT_OFF, pt_off_host, i)) return rc;
        if (int rc = sga_prefix_step("sga_object_partition", SLOT_OFF, slot_off_host, i)) return rc;
    }
    for (int i = 0; i < n_scans; ++i)
        SGA_CHECK_ARG(pt_off_host[i + 1] - pt_off_host[i] <= max_points && slot_off_host[i + 1] - slot_off_host[i] <= max_slots,
                      "sga_object_partition: scan %d is larger than max_points %d / max_slots %d", i, max_points, max_slots);
    {   // the kept objects' output ranges: inside [0, n_kept_points), disjoint
        std::vector<std::pair<long long, long long>> rng;
        for (int k = 0; k < total_slots; ++k) {
            const long long d = dest_off_host[k], c = counts_host[k];
            SGA_CHECK_ARG(c >= 0, "sga_object_partition: counts[%d] is negative", k);
            if (d < 0) continue;
            SGA_CHECK_ARG(d + c <= n_kept_points, "sga_object_partition: slot %d writes [%lld, %lld) of %d kept points", k, d, d + c, n_kept_points);
            if (c) rng.emplace_back(d, d + c);
        }
        std::sort(rng.begin(), rng.end());
        for (size_t i = 1; i < rng.size(); ++i)
            SGA_CHECK_ARG(rng[i].first >= rng[i - 1].second, "sga_object_partition: dest_off ranges overlap at output position %lld", rng[i].first);
    }
    if (n_scans == 0 || n_kept_points == 0 || max_points == 0 || max_slots == 0) return SGA_OK;              // nothing to write
    SGA_CHECK_ARG(pts && slot && pt_off && slot_off && dest_off && perm && pts_out && ws, "sga_object_partition: null pointer");
    SGA_CHECK_ARG(sga_aligned(4, pts, slot, pt_off, slot_off, dest_off, perm, pts_out, ws),
                  "sga_object_partition: misaligned pointer (32-bit arrays need 4 bytes)");
    const size_t need = sga_object_partition_ws_bytes(n_scans, max_points, max_slots);
    if (ws_bytes < need) {
        sga_set_error("sga_object_partition: workspace of %zu bytes, %zu needed", ws_bytes, need);
        return SGA_ERR_WORKSPACE;
    }
    SGA_CHECK_ARG(need / sizeof(int32_t) < ((size_t)1 << 31), "sga_object_partition: the tile table exceeds 2^31 counters; split the scan list");
    const long p_tiles = ((long)max_points + SG_TILE - 1) / SG_TILE;
    if (int rc = sga_check_grid("sga_object_partition", p_tiles, 1, n_scans, "split the scan list")) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    int* w = static_cast<int*>(ws);
    const unsigned grid = (unsigned)(p_tiles * n_scans);
    hipLaunchKernelGGL(tile_hist_kernel, dim3(grid), dim3(SG_THREADS), 0, st, slot, pt_off, slot_off, n_scans, total_points, total_slots, (int)p_tiles,
                       max_slots, w);
    const long cols = (long)n_scans * max_slots;
    hipLaunchKernelGGL(tile_scan_kernel, dim3((unsigned)((cols + SG_THREADS - 1) / SG_THREADS)), dim3(SG_THREADS), 0, st, pt_off, slot_off, n_scans,
                       total_points, total_slots, (int)p_tiles, max_slots, w);
    hipLaunchKernelGGL(tile_place_kernel, dim3(grid), dim3(64), 0, st, pts, slot, pt_off, slot_off, dest_off, n_scans, total_points, total_slots,
                       (int)p_tiles, max_slots, w, n_kept_points, perm, pts_out);
    SGA_CHECK_LAUNCH("sga_object_partition");
    return SGA_OK;
}

extern "C" int sga_graph_complete(const int32_t* node_off, const int32_t* pair_off, const int32_t* trip_off, const int32_t* edge_off, int n_graphs,
                                  const int32_t* pairs, const int32_t* rels, int none_id, int V, const int32_t* node_off_host,
                                  const int32_t* pair_off_host, const int32_t* trip_off_host, const int32_t* edge_off_host,
                                  const int32_t* pairs_host, const int32_t* rels_host, int64_t* edges, int32_t* n_edges, int32_t* bow, void* stream) {
    SGA_CHECK_ARG(n_graphs >= 0 && V >= 1, "sga_graph_complete: bad sizes (n_graphs %d, V %d)", n_graphs, V);
    SGA_CHECK_ARG(none_id >= 0 && none_id < V, "sga_graph_complete: the id of `none` (%d) is outside the vocabulary of %d", none_id, V);
    if (n_graphs == 0) return SGA_OK;
    long long tn = 0, tp = 0, tt = 0, te = 0;
    if (int rc = gc_offsets("node_off", node_off_host, n_graphs, &tn)) return rc;
    if (int rc = gc_offsets("pair_off", pair_off_host, n_graphs, &tp)) return rc;
    if (int rc = gc_offsets("trip_off", trip_off_host, n_graphs, &tt)) return rc;
    if (int rc = gc_offsets("edge_off", edge_off_host, n_graphs, &te)) return rc;
    SGA_CHECK_ARG(tn * V < (1LL << 31), "sga_graph_complete: %lld nodes x %d words exceed 2^31 counters; split the graph list", tn, V);
    for (int g = 0; g < n_graphs; ++g) {
        const long long N = node_off_host[g + 1] - node_off_host[g], P = pair_off_host[g + 1] - pair_off_host[g],
                        Tr = trip_off_host[g + 1] - trip_off_host[g], cap = edge_off_host[g + 1] - edge_off_host[g];
        SGA_CHECK_ARG(N <= GC_MAX_NODES, "sga_graph_complete: graph %d has %lld nodes, at most %d are supported", g, N, GC_MAX_NODES);
        SGA_CHECK_ARG(Tr >= P, "sga_graph_complete: graph %d lists %lld triples for %lld pairs (every pair comes from a triple)", g, Tr, P);
        SGA_CHECK_ARG(cap >= P + N * (N - 1), "sga_graph_complete: graph %d has room for %lld edges, %lld needed", g, cap, P + N * (N - 1));
        if (pairs_host)
            for (long long p = 2 * (long long)pair_off_host[g]; p < 2 * (long long)pair_off_host[g + 1]; ++p)
                SGA_CHECK_ARG(pairs_host[p] >= 0 && pairs_host[p] < N, "sga_graph_complete: graph %d lists node %d of %lld", g, pairs_host[p], N);
    }
    if (rels_host)
        for (long long t = 0; t < tt; ++t)
            SGA_CHECK_ARG(rels_host[t] >= 0 && rels_host[t] < V, "sga_graph_complete: relation %d at triple %lld is outside the vocabulary of %d",
                          rels_host[t], t, V);
    SGA_CHECK_ARG(node_off && pair_off && trip_off && edge_off && n_edges, "sga_graph_complete: null pointer");
    SGA_CHECK_ARG((pairs || tp == 0) && (rels || tt == 0) && (edges || te == 0) && (bow || tn == 0), "sga_graph_complete: null pointer");
    SGA_CHECK_ARG(sga_aligned(8, edges) && sga_aligned(4, node_off, pair_off, trip_off, edge_off, pairs, rels, n_edges, bow),
                  "sga_graph_complete: misaligned pointer (64-bit arrays need 8 bytes, 32-bit arrays 4)");
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (tn)
        if (int rc = sga_zero("sga_graph_complete", bow, (size_t)tn * V * sizeof(int32_t), st)) return rc;
    hipLaunchKernelGGL(graph_complete_kernel, dim3((unsigned)n_graphs), dim3(GC_THREADS), 0, st, node_off, pair_off, trip_off, edge_off, n_graphs, (int)tn,
                       (int)tp, (int)tt, (int)te, pairs, rels, none_id, V, reinterpret_cast<long long*>(edges), n_edges, bow);
    SGA_CHECK_LAUNCH("sga_graph_complete");
    return SGA_OK;
}

extern "C" int sga_bow_counts(const int32_t* rows, const int32_t* cols, int n, int T, int V, const int32_t* rows_host, const int32_t* cols_host,
                              int32_t* out, void* stream) {
    SGA_CHECK_ARG(n >= 0 && T >= 0 && V >= 0, "sga_bow_counts: negative count (n %d, T %d, V %d)", n, T, V);
    SGA_CHECK_ARG((long long)T * V < (1LL << 31), "sga_bow_counts: %d x %d exceed 2^31 counters", T, V);
    for (int i = 0; i < n; ++i) {
        if (rows_host) SGA_CHECK_ARG(rows_host[i] >= 0 && rows_host[i] < T, "sga_bow_counts: rows[%d] = %d is outside [0, %d)", i, rows_host[i], T);
        if (cols_host) SGA_CHECK_ARG(cols_host[i] >= 0 && cols_host[i] < V, "sga_bow_counts: cols[%d] = %d is outside [0, %d)", i, cols_host[i], V);
    }
    if (T == 0 || V == 0) return SGA_OK;                                                                     // nothing to write
    SGA_CHECK_ARG(out && (n == 0 || (rows && cols)), "sga_bow_counts: null pointer");
    SGA_CHECK_ARG(sga_aligned(4, rows, cols, out), "sga_bow_counts: misaligned pointer (32-bit arrays need 4 bytes)");
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (int rc = sga_zero("sga_bow_counts", out, (size_t)T * V * sizeof(int32_t), st)) return rc;
    if (n == 0) return SGA_OK;
    hipLaunchKernelGGL(bow_counts_kernel, dim3((unsigned)(((long)n + SG_THREADS - 1) / SG_THREADS)), dim3(SG_THREADS), 0, st, rows, cols, n, T, V, out);
    SGA_CHECK_LAUNCH("sga_bow_counts");
    return SGA_OK;
}
