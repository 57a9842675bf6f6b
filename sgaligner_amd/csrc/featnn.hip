// Batched exact-fp32 nearest-neighbour search in feature space on the fp32 matrix cores: the step between per-point descriptors and the
// [n, 6] correspondence array RANSAC reads (utils/open3d.py:137-170 registration_with_ransac_from_feats: Open3D matches every source
// descriptor to its nearest reference descriptor; src/engine/registration_evaluator.py:92-127 takes the same from GeoTransformer).
// A GEMM with an arg-min epilogue: 33 columns for FPFH, 256 for learned fine features, up to 10 000 x 10 000 rows per scan pair.
//
// Arithmetic contract.  For query row a and support row b_j the score is  s_j = n_j - 2 * dot_j  (one rounding: 2 * dot is exact), with
//   n_j   = |b_j|^2 as the fp32 chain n = fmaf(b_k, b_k, n), k ascending from n = 0 (featnn_norm_kernel, a pre-pass into the workspace);
//   dot_j = a . b_j on v_mfma_f32_32x32x2_f32, which is bit for bit a k-ordered fp32 fmaf chain from 0.  THE k ORDER: the columns go in
//           chunks of SGA_KC = 32, chunks ascending; inside a chunk in four groups of 8, groups ascending; inside group g of the chunk at k0
//           the four MFMAs r = 0..3 each add k = k0 + 8g + r (lower lane half) and then k = k0 + 8g + 4 + r (upper lane half), i.e.
//           k0 + 8g + {0, 4, 1, 5, 2, 6, 3, 7}  (mfma_tiles.h: one ds_read_b128 per operand feeds four MFMAs).  Columns past C inside the
//           last chunk are zero on both sides and leave the chain unchanged.
// The score is therefore a pure function of the two rows.  out_idx = arg-min_j s_j, the LOWEST j among exactly equal scores; a NaN score
// never wins (strict < against a running best that starts at +inf), so a query none of whose scores is below +inf -- an empty support, or
// nothing but NaN / overflowed rows -- gets -1.  out_d2 is recomputed for the chosen row alone in fp64:  sum_k (double(a_k) - double(b_k))^2,
// k ascending, every operation rounded on its own (explicit order AND -ffp-contract=off for this file, _build.FILE_FLAGS); +inf with -1.
//
// Layout.  A workgroup is one entry (job, query tile, chunk) of the caller's tile list: 4 waves, 128 queries (32 per wave), one chunk of
// the support walked in tiles of 128 rows, ascending.  Queries sit on the MFMA's B rows, so the C/D column (lane & 31) is the query and
// the 16 accumulator registers of each of the four 32-row support sub-tiles are support rows (row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)).
// Every lane reduces its 64 scores of a support tile in registers, in ascending row order with a strict <; the tile loop has no cross-lane
// traffic.  The two lane halves combine once at the end by (score, index).  Both operands are staged per 32-column chunk through LDS
// ([row][36] floats: conflict-free ds_read_b128), two stages deep, the next chunk's global loads in flight while this one is multiplied;
// rows past the chunk's end are zero-filled and carry the norm +inf, so they never win.
// Jobs with ns <= chunk write out_idx directly; larger ones write per-chunk (score, idx) partials that featnn_finish_kernel folds in
// ascending chunk order (strict <: the lower index of equal scores stays).  That kernel also computes out_d2.  No atomics anywhere.
#include <math.h>

#include "mfma_tiles.h"
#include "pair_jobs.h"

namespace {

constexpr int FN_THREADS = 256;
constexpr int FN_QTILE = 128;                     // queries per workgroup: 32 per wave
constexpr int FN_NT = 4;                          // 32-row support sub-tiles per staged tile
constexpr int FN_STILE = 32 * FN_NT;              // support rows per staged tile

// |b|^2 of every packed row: n = fmaf(b_k, b_k, n), k ascending.
__global__ __launch_bounds__(FN_THREADS) void featnn_norm_kernel(const float* __restrict__ feats, int C, int total_rows, float* __restrict__ norms) {
    const long long i = (long long)blockIdx.x * FN_THREADS + threadIdx.x;
    if (i >= total_rows) return;
    const f32x4* p = reinterpret_cast<const f32x4*>(feats + (size_t)i * C);
    float n = 0.f;
    for (int k = 0; k < C / 4; ++k) {
        const f32x4 v = p[k];
#pragma unroll
        for (int e = 0; e < 4; ++e) n = fmaf(v[e], v[e], n);
    }
    norms[i] = n;
}

// One 32-column chunk of a 128-row support tile and of the 128-row query tile on their way from global memory to LDS: four float4 of each
// per lane, in lds_load_rows' element order (mfma_tiles.h), held in registers while the previous chunk is multiplied.
struct FNStage { f32x4 a[4], b[4]; };
constexpr int FN_V = SGA_KC / 4;                  // float4 per staged row

__device__ __forceinline__ void fn_fetch(FNStage& st, const float* __restrict__ S, const float* __restrict__ Q, int C, int t0, int c1, int qb, int nq,
                                         int k0, int tid) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int v = tid + e * FN_THREADS, r = v / FN_V, gc = k0 + (v % FN_V) * 4;
        const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
        const long long sr = (long long)t0 + r, qr = (long long)qb + r;
        st.a[e] = (sr < c1 && gc < C) ? *reinterpret_cast<const f32x4*>(S + (size_t)sr * C + gc) : zero;      // past the end: zero-filled
        st.b[e] = (qr < nq && gc < C) ? *reinterpret_cast<const f32x4*>(Q + (size_t)qr * C + gc) : zero;
    }
}

__device__ __forceinline__ void fn_put(const FNStage& st, float* __restrict__ sa, float* __restrict__ sb, int tid) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int v = tid + e * FN_THREADS, o = (v / FN_V) * SGA_LDS_STRIDE + (v % FN_V) * 4;
        *reinterpret_cast<f32x4*>(sa + o) = st.a[e];
        *reinterpret_cast<f32x4*>(sb + o) = st.b[e];
    }
}

__global__ __launch_bounds__(FN_THREADS) void featnn_kernel(const float* __restrict__ feats, int C, const int* __restrict__ off, int n_sets,
                                                            int total_rows, const int* __restrict__ pairs, int n_pairs,
                                                            const int* __restrict__ out_off, const int* __restrict__ tiles, int total_queries,
                                                            int n_chunks, int chunk, const float* __restrict__ norms, int* __restrict__ out_i,
                                                            float* __restrict__ ws_s, int* __restrict__ ws_i) {
    // two stages: chunk i + 1 is written while chunk i is read, one barrier per chunk; the norms alternate per support tile
    __shared__ __attribute__((aligned(16))) float sa[2][FN_STILE * SGA_LDS_STRIDE];
    __shared__ __attribute__((aligned(16))) float sb[2][FN_QTILE * SGA_LDS_STRIDE];
    __shared__ __attribute__((aligned(16))) float sn[2][FN_STILE];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int job = tiles[3 * (size_t)blockIdx.x], qt = tiles[3 * (size_t)blockIdx.x + 1], c = tiles[3 * (size_t)blockIdx.x + 2];
    const SgaPairJob J = sga_pair_job(off, n_sets, total_rows, pairs, n_pairs, out_off, total_queries, job);
    if (!J.ok || qt < 0 || c < 0) return;
    if ((long long)qt * FN_QTILE >= J.nq) return;
    const int qb = qt * FN_QTILE;
    const int my_chunks = sga_chunks(J.ns, chunk);                           // empty support: one pass that writes -1
    if (c >= my_chunks || c >= n_chunks) return;
    const bool direct = my_chunks == 1;
    if (!direct && (!ws_s || !ws_i)) return;
    const int c0 = c * chunk, c1 = (int)min((long long)J.ns, (long long)c0 + chunk);     // c < my_chunks: c * chunk < ns

    const float* Q = feats + (size_t)J.q0 * C;
    const float* S = feats + (size_t)J.s0 * C;
    const int b_off = (wave * 32 + (lane & 31)) * SGA_LDS_STRIDE;
    const int h = lane >> 5;
    float best = INFINITY;
    int bi = -1;
    FNStage st;
    if (c0 < c1) fn_fetch(st, S, Q, C, c0, c1, qb, J.nq, 0, tid);
    int cur = 0, par = 0;                                                    // LDS stage of this chunk, norm buffer of this tile
    for (long long t0l = c0; t0l < c1; t0l += FN_STILE, par ^= 1) {
        const int t0 = (int)t0l;
        f32x16 acc[FN_NT];
        zero_acc<FN_NT>(acc);
        for (int k0 = 0; k0 < C; k0 += SGA_KC, cur ^= 1) {
            // stage `cur` was last read two chunks ago, and every wave has passed the barrier of the chunk between
            fn_put(st, sa[cur], sb[cur], tid);
            if (k0 == 0 && tid < FN_STILE) sn[par][tid] = t0l + tid < c1 ? norms[(size_t)J.s0 + t0 + tid] : INFINITY;
            const bool last_k = k0 + SGA_KC >= C;
            const long long nt = last_k ? t0l + FN_STILE : t0l;
            if (nt < c1) fn_fetch(st, S, Q, C, (int)nt, c1, qb, J.nq, last_k ? 0 : k0 + SGA_KC, tid);      // in flight while this chunk is multiplied
            __syncthreads();
            mfma_chunk<FN_NT>(acc, sa[cur], sb[cur] + b_off, lane);
        }
        // this lane's 64 support rows of the tile, ascending: t, then g = r >> 2, then r & 3
#pragma unroll
        for (int t = 0; t < FN_NT; ++t) {
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int row = t * 32 + 8 * g + 4 * h;
                const f32x4 n4 = *reinterpret_cast<const f32x4*>(sn[par] + row);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float s = n4[e] - 2.0f * acc[t][4 * g + e];
                    if (s < best) { best = s; bi = t0 + row + e; }          // strict: the first (lowest) index of a minimum stays
                }
            }
        }
    }
    // the two halves of the wave hold the same query over interleaved rows: the lower (score, index) stays
    const float os = __shfl_xor(best, 32, 64);
    const int oi = __shfl_xor(bi, 32, 64);
    if (os < best || (os == best && oi < bi)) { best = os; bi = oi; }
    const int i = qb + wave * 32 + lane;
    if (lane >= 32 || i >= J.nq) return;
    if (direct) {
        out_i[(size_t)J.oo + i] = bi;
    } else {
        const size_t w = (size_t)c * total_queries + J.oo + i;
        ws_s[w] = best;
        ws_i[w] = bi;
    }
}

// One entry (job, query tile, 0) of the tile list per workgroup: fold a split job's chunks in ascending order, then the fp64 distance to the
// chosen row.
__global__ __launch_bounds__(FN_QTILE) void featnn_finish_kernel(const float* __restrict__ feats, int C, const int* __restrict__ off, int n_sets,
                                                                 int total_rows, const int* __restrict__ pairs, int n_pairs,
                                                                 const int* __restrict__ out_off, const int* __restrict__ tiles, int total_queries,
                                                                 int n_chunks, int chunk, int* __restrict__ out_i, double* __restrict__ out_d,
                                                                 const float* __restrict__ ws_s, const int* __restrict__ ws_i) {
    const int job = tiles[3 * (size_t)blockIdx.x], qt = tiles[3 * (size_t)blockIdx.x + 1], c = tiles[3 * (size_t)blockIdx.x + 2];
    const SgaPairJob J = sga_pair_job(off, n_sets, total_rows, pairs, n_pairs, out_off, total_queries, job);
    if (!J.ok || qt < 0 || c != 0) return;
    const long long il = (long long)qt * FN_QTILE + threadIdx.x;
    if (il >= J.nq) return;
    const int i = (int)il;
    const int my_chunks = sga_chunks(J.ns, chunk);
    int bi = -1;
    if (my_chunks > 1) {
        if (!ws_s || !ws_i) return;
        float best = INFINITY;
        for (int k = 0; k < min(my_chunks, n_chunks); ++k) {               // never past what featnn_kernel wrote
            const size_t w = (size_t)k * total_queries + J.oo + i;
            const float s = ws_s[w];
            if (s < best) { best = s; bi = ws_i[w]; }                       // ascending chunks, strict: the lower index of equal scores stays
        }
        out_i[(size_t)J.oo + i] = bi;
    } else {
        bi = out_i[(size_t)J.oo + i];
    }
    double d2 = INFINITY;
    if (bi >= 0 && bi < J.ns) {
        const f32x4* a = reinterpret_cast<const f32x4*>(feats + ((size_t)J.q0 + i) * C);
        const f32x4* b = reinterpret_cast<const f32x4*>(feats + ((size_t)J.s0 + bi) * C);
        d2 = 0.0;
        for (int k = 0; k < C / 4; ++k) {
            const f32x4 x = a[k], y = b[k];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const double d = __dsub_rn((double)x[e], (double)y[e]);
                d2 = __dadd_rn(d2, __dmul_rn(d, d));
            }
        }
    }
    out_d[(size_t)J.oo + i] = d2;
}

inline size_t fn_norm_bytes(int total_rows) { return ((size_t)total_rows * sizeof(float) + 7) / 8 * 8; }

}  // namespace

extern "C" size_t sga_featnn_workspace_bytes(int total_rows, int total_queries, int max_support, int chunk) {
    if (total_rows <= 0 || total_queries <= 0 || chunk <= 0) return 0;
    const long nc = sga_chunks(max_support, chunk);                     // the norms are needed even when every support is empty
    return fn_norm_bytes(total_rows) + (nc <= 1 ? 0 : (size_t)nc * (size_t)total_queries * (sizeof(float) + sizeof(int32_t)));
}

extern "C" int sga_featnn_search(const float* feats, int C, const int32_t* offsets, int n_sets, int total_rows, const int32_t* pairs, int n_pairs,
                                 const int32_t* out_offsets, const int32_t* tiles, int n_tiles, int n_query_tiles, int total_queries,
                                 int max_queries, int max_support, int chunk, const int32_t* offsets_host, const int32_t* pairs_host,
                                 const int32_t* tiles_host, int32_t* out_idx, double* out_d2, void* workspace, size_t workspace_bytes,
                                 void* stream) {
    const char* who = "sga_featnn_search";
    SGA_CHECK_ARG(n_sets >= 0 && total_rows >= 0 && n_pairs >= 0 && total_queries >= 0 && max_queries >= 0 && max_support >= 0 && n_tiles >= 0 &&
                      n_query_tiles >= 0,
                  "sga_featnn_search: negative count (n_sets %d, total_rows %d, n_pairs %d, total_queries %d, max_queries %d, max_support %d, "
                  "n_tiles %d, n_query_tiles %d)",
                  n_sets, total_rows, n_pairs, total_queries, max_queries, max_support, n_tiles, n_query_tiles);
    SGA_CHECK_ARG(C >= 1 && C % 4 == 0, "sga_featnn_search: C must be a positive multiple of 4 (got %d); pad the rows with zero columns", C);
    if (int rc = sga_check_chunked(who, chunk, max_queries, total_queries)) return rc;
    SGA_CHECK_ARG(n_query_tiles <= n_tiles, "sga_featnn_search: n_query_tiles %d exceeds n_tiles %d", n_query_tiles, n_tiles);
    if (n_pairs == 0 || total_queries == 0 || max_queries == 0 || n_tiles == 0) return SGA_OK;               // nothing to write
    SGA_CHECK_ARG(offsets && pairs && out_offsets && tiles && out_idx && out_d2, "sga_featnn_search: null pointer");
    SGA_CHECK_ARG(feats || total_rows == 0, "sga_featnn_search: null feature array");
    SGA_CHECK_ARG(sga_aligned(16, feats) && sga_aligned(8, out_d2, workspace) && sga_aligned(4, offsets, pairs, out_offsets, tiles, out_idx),
                  "sga_featnn_search: misaligned pointer (feats needs 16 bytes, fp64 arrays and the workspace 8, int32 arrays 4)");
    const SgaPrefix OFFSETS{"offsets", "decrease", "set", "total_rows", nullptr, nullptr};
    if (int rc = sga_check_prefix(who, OFFSETS, offsets_host, n_sets, total_rows, SGA_ANY)) return rc;
    if (int rc = sga_check_pairs(who, "set", pairs_host, n_pairs, offsets_host, n_sets, max_queries, max_support)) return rc;
    const long n_chunks = sga_chunks(max_support, chunk);
    if (tiles_host) {
        for (int t = 0; t < n_tiles; ++t) {
            const int job = tiles_host[3 * (size_t)t], qt = tiles_host[3 * (size_t)t + 1], c = tiles_host[3 * (size_t)t + 2];
            SGA_CHECK_ARG(job >= 0 && job < n_pairs && qt >= 0 && (long)qt * FN_QTILE < max_queries && c >= 0 && c < n_chunks,
                          "sga_featnn_search: tile %d = (job %d, query tile %d, chunk %d) is out of range", t, job, qt, c);
            SGA_CHECK_ARG((t < n_query_tiles) == (c == 0), "sga_featnn_search: tile %d: the first n_query_tiles entries, and only they, have chunk 0", t);
        }
    }
    if (int rc = sga_check_grid(who, n_tiles, 1, 1, "split the job list")) return rc;
    if (int rc = sga_check_grid(who, ((long)total_rows + FN_THREADS - 1) / FN_THREADS, 1, 1, "split the job list")) return rc;
    const size_t need = sga_featnn_workspace_bytes(total_rows, total_queries, max_support, chunk);
    if (int rc = sga_check_workspace(who, need, workspace, workspace_bytes)) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    float* norms = static_cast<float*>(workspace);
    float* ws_s = n_chunks > 1 ? reinterpret_cast<float*>(static_cast<char*>(workspace) + fn_norm_bytes(total_rows)) : nullptr;
    int* ws_i = ws_s ? reinterpret_cast<int*>(ws_s + (size_t)n_chunks * total_queries) : nullptr;
    if (total_rows > 0)
        hipLaunchKernelGGL(featnn_norm_kernel, dim3((unsigned)(((long)total_rows + FN_THREADS - 1) / FN_THREADS)), dim3(FN_THREADS), 0, s, feats, C,
                           total_rows, norms);
    hipLaunchKernelGGL(featnn_kernel, dim3((unsigned)n_tiles), dim3(FN_THREADS), 0, s, feats, C, offsets, n_sets, total_rows, pairs, n_pairs,
                       out_offsets, tiles, total_queries, (int)n_chunks, chunk, norms, out_idx, ws_s, ws_i);
    if (n_query_tiles > 0)
        hipLaunchKernelGGL(featnn_finish_kernel, dim3((unsigned)n_query_tiles), dim3(FN_QTILE), 0, s, feats, C, offsets, n_sets, total_rows, pairs,
                           n_pairs, out_offsets, tiles, total_queries, (int)n_chunks, chunk, out_idx, out_d2, ws_s, ws_i);
    SGA_CHECK_LAUNCH("sga_featnn_search");
    return SGA_OK;
}
