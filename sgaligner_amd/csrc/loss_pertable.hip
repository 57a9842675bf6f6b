// Per-table form of the contrastive / alignment loss kernels (contrastive.hip describes the loss): one launch per embedding table of any
// width, the joint table multiplied like every other.  ops.ContrastiveTermsFn runs it where the fused kernels do not apply: a single
// table (M = 1), tables wider than 104 columns, a joint table that is not the fusion of the others, MFMA mode 'f16'.
//   sweep / sweep_fast (Dp <= 128) / sweep_coef (wide tables: coefficient stash + GEMMs)   anchors x negatives sums and gradient
//   anchor<fwd|bwd[, PRE]>                                                                  anchors x anchors terms and dL/dS stash
//   stash_gemm                                                                              dZ from the stash when sga_gemm's alignment fails
#include "mfma_tiles.h"

#include "loss_math.h"
#include "sweep_groups.h"
#include "wide16_api.h"

// gemm.hip (include/sgaligner_hip.h): the stash gradient of the anchors x anchors backward runs on the GEMM kernels
extern "C" int sga_gemm(int transA, int transB, int M, int N, int K, const void* A, long lda, int a_is_f64, const float* B,
                        long ldb, float* C, long ldc, const float* bias, int accumulate, void* stream);

namespace {

constexpr int CT_THREADS = 256;
constexpr int CT_MAXT = 9;            // modalities (<= 8) + joint
// ------------------------------------------------------------------------------------------------
// owner-stationary sweeps over (owner rows) x (other rows): pass-1 sums and the negatives' gradient
// ------------------------------------------------------------------------------------------------
struct SweepArgs {
    const float* Z; int Dp; int ngroups; SweepGroup grp[4];
    float k0, k1;                   // log2(e)/tau for the two temperatures
    float it0, it1;                 // 1/tau
    double* sums;                   // [8]  (fam*2 + temp)            (SUM mode: output)
    const double* gs;               // [8]  dL/d(sums)                (GRAD mode: input)
    float* dZ;                      // [R][Dp]                        (GRAD mode: atomic accumulate)
    int col0;                       // first gradient column of this pass (GRAD, Dp > NCT*32)
};

template <int NJT, int NCT, bool GRAD>
__global__ __launch_bounds__(CT_THREADS) void sweep_kernel(SweepArgs a) {
    constexpr int OT = NJT * 32;                      // other rows per step
    constexpr int GW = NCT * 32;                      // gradient columns per pass
    extern __shared__ __attribute__((aligned(16))) float lds[];    // max(S chunks, gradient tile): sweep_lds_bytes()
    float* own_s = lds;
    float* oth_s = lds + 128 * SGA_LDS_STRIDE;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5;
    int g = 0;
#pragma unroll
    for (int i = 1; i < 4; ++i) if (i < a.ngroups && (int)blockIdx.x >= a.grp[i].blk0) g = i;
    const SweepGroup& grp = a.grp[g];
    const int own0 = grp.own0 + ((int)blockIdx.x - grp.blk0) * 128;
    const int own_end = grp.own0 + grp.nown;
    const int my_i = own0 + wave * 32 + (lane & 31);

    f32x16 gacc[GRAD ? NCT : 1];
    if (GRAD) zero_acc<GRAD ? NCT : 1>(gacc);
    double dsum[2][2] = {{0.0, 0.0}, {0.0, 0.0}};

#pragma unroll
    for (int sg = 0; sg < 2; ++sg) {
        if (sg >= grp.nseg) break;
        const SweepSeg seg = grp.seg[sg];
        float c0 = 0.f, c1 = 0.f;
        if (GRAD) { c0 = (float)(a.gs[seg.fam * 2 + 0] * (double)a.it0); c1 = (float)(a.gs[seg.fam * 2 + 1] * (double)a.it1); }
        const int ntile = (seg.n + OT - 1) / OT;
        for (int jt = blockIdx.y; jt < ntile; jt += gridDim.y) {
            const int j0 = seg.row0 + jt * OT, j_end = seg.row0 + seg.n;
            f32x16 sacc[NJT];
            zero_acc<NJT>(sacc);
            for (int k0 = 0; k0 < a.Dp; k0 += SGA_KC) {
                __syncthreads();
                lds_load_rows<128, CT_THREADS>(own_s, a.Z, a.Dp, own0, own_end, k0, a.Dp, tid);
                lds_load_rows<OT, CT_THREADS>(oth_s, a.Z, a.Dp, j0, j_end, k0, a.Dp, tid);
                __syncthreads();
                mfma_chunk<NJT>(sacc, oth_s, own_s + (wave * 32 + (lane & 31)) * SGA_LDS_STRIDE, lane);
            }
            if (!GRAD) {
                float p0 = 0.f, p1 = 0.f;
                const bool iv = my_i < own_end;
#pragma unroll
                for (int t = 0; t < NJT; ++t)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const float okf = (iv && (j0 + t * 32 + mfma32_row(r, h) < j_end)) ? 1.f : 0.f;
                        p0 = fmaf(okf, fexp2(sacc[t][r] * a.k0), p0);
                        p1 = fmaf(okf, fexp2(sacc[t][r] * a.k1), p1);
                    }
                dsum[sg][0] += (double)p0;
                dsum[sg][1] += (double)p1;
            } else {
                // coefficient dL/d(dot) = sum_temp dL/ds * exp(dot/tau)/tau, in place (A-operand layout)
#pragma unroll
                for (int t = 0; t < NJT; ++t)
#pragma unroll
                    for (int r = 0; r < 16; ++r)
                        sacc[t][r] = c0 * fexp2(sacc[t][r] * a.k0) + c1 * fexp2(sacc[t][r] * a.k1);
                __syncthreads();
                // stage the other rows' gradient columns [OT][GW] (zero beyond valid rows / Dp)
                for (int e = tid; e < OT * (GW / 4); e += CT_THREADS) {
                    const int r = e / (GW / 4), c = (e % (GW / 4)) * 4;
                    const int gr = j0 + r, gc = a.col0 + c;
                    f32x4 v = {0.f, 0.f, 0.f, 0.f};
                    if (gr < j_end && gc < a.Dp) v = *reinterpret_cast<const f32x4*>(a.Z + (size_t)gr * a.Dp + gc);
                    *reinterpret_cast<f32x4*>(lds + r * GW + c) = v;
                }
                __syncthreads();
#pragma unroll
                for (int t = 0; t < NJT; ++t)
#pragma unroll
                    for (int s = 0; s < 16; ++s) {
                        const float av = sacc[t][s];
                        const float* brow = lds + (t * 32 + mfma32_row(s, h)) * GW + (lane & 31);
#pragma unroll
                        for (int ct = 0; ct < NCT; ++ct)
                            gacc[ct] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, brow[ct * 32], gacc[ct], 0, 0, 0);
                    }
            }
        }
    }
    if (!GRAD) {
#pragma unroll
        for (int sg = 0; sg < 2; ++sg)
#pragma unroll
            for (int tt = 0; tt < 2; ++tt) {
                const double v = wave_sum_d(dsum[sg][tt]);
                if (lane == 0 && sg < grp.nseg && v != 0.0) atomicAdd(a.sums + 8 + my_slot() * 8 + grp.seg[sg].fam * 2 + tt, v);
            }
    } else {
        // gacc[ct][r] = dOwner[wave*32 + row(r,h)][col0 + ct*32 + (lane&31)]
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct) {
            const int d = a.col0 + ct * 32 + (lane & 31);
            if (d < a.Dp) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int i = own0 + wave * 32 + mfma32_row(r, h);
                    if (i < own_end) atomicAdd(a.dZ + (size_t)i * a.Dp + d, gacc[ct][r]);
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------
// Wide tables (Dp > 128: 1024-d modality tables, 300-/3072-d joint tables on the general path).  sweep_kernel<.,10,true> covers 320
// gradient columns per pass and recomputes the K = Dp similarity tile in every pass (Dp = 3072: 10 passes, 5.5x the necessary FLOPs;
// 293 of the 340 ms of a BASELINE configs[4]-shaped step).  For wide rows S is the expensive part, so the trade of the 100-d path
// is reversed: ONE anchor-owner sweep computes S and the coefficient c_ij = dL/dS_ij and writes it, transposed, to a stash
// Ct[g][j - n1][i - own0] (lane = anchor: 128-byte stores); both gradients are then plain GEMMs on the stash,
//   dZ[anchors] += Ct^T Z[negatives]   (gemm_tn)        dZ[negatives] += Ct Z[anchors]   (gemm_nn),
// so S is computed once instead of 2 x passes times.  The stash is bounded by the caller's workspace: anchor-row blocks.
// ------------------------------------------------------------------------------------------------
struct CoefArgs {
    const float* Z; int Dp; SweepGroup grp[2];
    float k0, k1, it0, it1;
    const double* gs;               // [8] dL/d(sums)
    float* stash[2];                // per anchor group: [J1 + J2][ld] (negative-major)
    int ld, n1;                     // stash row length (anchors in this block), first negative row of the packed table
};

template <int NJT>
__global__ __launch_bounds__(CT_THREADS) void sweep_coef_kernel(CoefArgs a) {
    constexpr int OT = NJT * 32;
    __shared__ __attribute__((aligned(16))) float own_s[128 * SGA_LDS_STRIDE];
    __shared__ __attribute__((aligned(16))) float oth_s[OT * SGA_LDS_STRIDE];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5;
    const int g = ((int)blockIdx.x >= a.grp[1].blk0 && a.grp[1].nown > 0) ? 1 : 0;
    const SweepGroup& grp = a.grp[g];
    const int own0 = grp.own0 + ((int)blockIdx.x - grp.blk0) * 128;
    const int own_end = grp.own0 + grp.nown;
    const int my_i = own0 + wave * 32 + (lane & 31);
    float* __restrict__ st = a.stash[g];
#pragma unroll
    for (int sg = 0; sg < 2; ++sg) {
        const SweepSeg seg = grp.seg[sg];
        const float c0 = (float)(a.gs[seg.fam * 2 + 0] * (double)a.it0), c1 = (float)(a.gs[seg.fam * 2 + 1] * (double)a.it1);
        const int ntile = (seg.n + OT - 1) / OT;
        for (int jt = blockIdx.y; jt < ntile; jt += gridDim.y) {
            const int j0 = seg.row0 + jt * OT, j_end = seg.row0 + seg.n;
            f32x16 sacc[NJT];
            zero_acc<NJT>(sacc);
            for (int k0 = 0; k0 < a.Dp; k0 += SGA_KC) {
                __syncthreads();
                lds_load_rows<128, CT_THREADS>(own_s, a.Z, a.Dp, own0, own_end, k0, a.Dp, tid);
                lds_load_rows<OT, CT_THREADS>(oth_s, a.Z, a.Dp, j0, j_end, k0, a.Dp, tid);
                __syncthreads();
                mfma_chunk<NJT>(sacc, oth_s, own_s + (wave * 32 + (lane & 31)) * SGA_LDS_STRIDE, lane);
            }
            if (my_i < own_end) {
#pragma unroll
                for (int t = 0; t < NJT; ++t)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int j = j0 + t * 32 + mfma32_row(r, h);
                        if (j < j_end) st[(size_t)(j - a.n1) * a.ld + (my_i - grp.own0)] = c0 * fexp2(sacc[t][r] * a.k0) + c1 * fexp2(sacc[t][r] * a.k1);
                    }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------
// Fast path of the sweeps for Dp <= 128 (emb_dim = 100 -> Dp = 104): the wave's 32 owner rows live in
// registers for the whole sweep (NQ float4 per lane = the MFMA B operand of every S tile), and each
// 128-row "other" tile is staged ONCE into LDS as full rows and serves both the S tiles (ds_read_b128
// along k) and the gradient GEMM (ds_read_b32 along the columns): one global->LDS pass and two barriers
// per tile instead of one per 32-wide K chunk and a second staging for the gradient.
// ------------------------------------------------------------------------------------------------
template <int NQ, bool GRAD>
__global__ __launch_bounds__(CT_THREADS) void sweep_fast_kernel(SweepArgs a) {
    constexpr int DP = NQ * 8;
    constexpr int STR = DP + 4;                         // (DP+4)/4 odd -> conflict-free ds_read_b128 over 16 rows
    constexpr int NJT = 4, OT = 128, NCT = 4;
    extern __shared__ __attribute__((aligned(16))) float lds[];     // [OT][STR] + 32 floats of slack

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5;
    int g = 0;
#pragma unroll
    for (int i = 1; i < 4; ++i) if (i < a.ngroups && (int)blockIdx.x >= a.grp[i].blk0) g = i;
    const SweepGroup& grp = a.grp[g];
    const int own0 = grp.own0 + ((int)blockIdx.x - grp.blk0) * 128;
    const int own_end = grp.own0 + grp.nown;
    const int my_i = own0 + wave * 32 + (lane & 31);

    // owner rows -> registers (zero for rows past the group's end)
    f32x4 own[NQ];
    {
        const float* src = a.Z + (size_t)(my_i < own_end ? my_i : own0) * DP + 4 * h;
        const float msk = my_i < own_end ? 1.f : 0.f;
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            f32x4 v = *reinterpret_cast<const f32x4*>(src + 8 * q);
            own[q] = v * msk;
        }
    }
    f32x16 gacc[GRAD ? NCT : 1];
    if (GRAD) zero_acc<GRAD ? NCT : 1>(gacc);
    double dsum[2][2] = {{0.0, 0.0}, {0.0, 0.0}};

#pragma unroll
    for (int sg = 0; sg < 2; ++sg) {
        if (sg >= grp.nseg) break;
        const SweepSeg seg = grp.seg[sg];
        float c0 = 0.f, c1 = 0.f;
        if (GRAD) { c0 = (float)(a.gs[seg.fam * 2 + 0] * (double)a.it0); c1 = (float)(a.gs[seg.fam * 2 + 1] * (double)a.it1); }
        const int ntile = (seg.n + OT - 1) / OT;
        for (int jt = blockIdx.y; jt < ntile; jt += gridDim.y) {
            const int j0 = seg.row0 + jt * OT, j_end = seg.row0 + seg.n;
            __syncthreads();                              // previous tile fully consumed
            for (int e = tid; e < OT * (DP / 4); e += CT_THREADS) {
                const int r = e / (DP / 4), c = (e % (DP / 4)) * 4;
                f32x4 v = {0.f, 0.f, 0.f, 0.f};
                if (j0 + r < j_end) v = *reinterpret_cast<const f32x4*>(a.Z + (size_t)(j0 + r) * DP + c);
                *reinterpret_cast<f32x4*>(lds + r * STR + c) = v;
            }
            __syncthreads();
            // ---- S tiles: lane = owner row, registers = other rows
            f32x16 sacc[NJT];
            zero_acc<NJT>(sacc);
            const float* ap = lds + (lane & 31) * STR + 4 * h;
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
#pragma unroll
                for (int t = 0; t < NJT; ++t) {
                    const f32x4 av = *reinterpret_cast<const f32x4*>(ap + t * 32 * STR + 8 * q);
#pragma unroll
                    for (int r = 0; r < 4; ++r) sacc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[r], own[q][r], sacc[t], 0, 0, 0);
                }
            }
            if (!GRAD) {
                float p0 = 0.f, p1 = 0.f;
                const bool iv = my_i < own_end;
#pragma unroll
                for (int t = 0; t < NJT; ++t)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const float okf = (iv && (j0 + t * 32 + mfma32_row(r, h) < j_end)) ? 1.f : 0.f;
                        p0 = fmaf(okf, fexp2(sacc[t][r] * a.k0), p0);
                        p1 = fmaf(okf, fexp2(sacc[t][r] * a.k1), p1);
                    }
                dsum[sg][0] += (double)p0;
                dsum[sg][1] += (double)p1;
            } else {
#pragma unroll
                for (int t = 0; t < NJT; ++t)
#pragma unroll
                    for (int r = 0; r < 16; ++r)
                        sacc[t][r] = c0 * fexp2(sacc[t][r] * a.k0) + c1 * fexp2(sacc[t][r] * a.k1);
                // ---- gradient GEMM straight from the accumulators (rows past j_end are zero in LDS)
#pragma unroll
                for (int t = 0; t < NJT; ++t)
#pragma unroll
                    for (int s = 0; s < 16; ++s) {
                        const float av = sacc[t][s];
                        const float* brow = lds + (t * 32 + mfma32_row(s, h)) * STR + (lane & 31);
#pragma unroll
                        for (int ct = 0; ct < NCT; ++ct)
                            gacc[ct] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, brow[ct * 32], gacc[ct], 0, 0, 0);
                    }
            }
        }
    }
    if (!GRAD) {
#pragma unroll
        for (int sg = 0; sg < 2; ++sg)
#pragma unroll
            for (int tt = 0; tt < 2; ++tt) {
                const double v = wave_sum_d(dsum[sg][tt]);
                if (lane == 0 && sg < grp.nseg && v != 0.0) atomicAdd(a.sums + 8 + my_slot() * 8 + grp.seg[sg].fam * 2 + tt, v);
            }
    } else {
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct) {
            const int d = ct * 32 + (lane & 31);
            if (d < DP) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int i = own0 + wave * 32 + mfma32_row(r, h);
                    if (i < own_end) atomicAdd(a.dZ + (size_t)i * DP + d, gacc[ct][r]);
                }
            }
        }
    }
}

template <int NJT, int NCT, bool GRAD>
static void launch_sweep(const SweepArgs& a, int nblk, int gy, hipStream_t s) {
    const size_t sf = (size_t)(128 + NJT * 32) * SGA_LDS_STRIDE, gf = GRAD ? (size_t)NJT * 32 * NCT * 32 : 0;
    const size_t lds = (sf > gf ? sf : gf) * sizeof(float);
    auto k = sweep_kernel<NJT, NCT, GRAD>;
    hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(k, dim3(nblk, gy), dim3(CT_THREADS), lds, s, a);
}

template <int NQ, bool GRAD>
static void launch_sweep_fast(const SweepArgs& a, int nblk, int gy, hipStream_t s) {
    const size_t lds = (size_t)(128 * (NQ * 8 + 4) + 32) * sizeof(float);
    auto k = sweep_fast_kernel<NQ, GRAD>;
    hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(k, dim3(nblk, gy), dim3(CT_THREADS), lds, s, a);
}

// fp16 staging of the general-width anchors x anchors kernel: the same LDS tiles hold [rows][64 halfs + 8 pad] (144 B = the fp32 tiles' 36
// floats per row: conflict-free ds_read_b128), a K chunk is 64 columns = 4 steps of v_mfma_f32_32x32x16_f16 (lane: row lane & 31, k slots
// 8 (lane >> 5) .. + 7 of each step)
typedef _Float16 ak_f16x8 __attribute__((ext_vector_type(8)));
template <int NROWS, int NTHREADS>
__device__ __forceinline__ void lds_load_rows_h(float* __restrict__ tile, const _Float16* __restrict__ g, int ld, int row0, int nrows, int k0,
                                                int ncols, int tid) {
    unsigned char* t8 = reinterpret_cast<unsigned char*>(tile);
#pragma unroll
    for (int e = tid; e < NROWS * 8; e += NTHREADS) {
        const int r = e >> 3, c = (e & 7) * 8;
        ak_f16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
        const int gr = row0 + r, gc = k0 + c;
        if (gr < nrows && gc < ncols) v = *reinterpret_cast<const ak_f16x8*>(g + (size_t)gr * ld + gc);     // ncols % 8 == 0
        *reinterpret_cast<ak_f16x8*>(t8 + r * 144 + c * 2) = v;
    }
}
template <int NT>
__device__ __forceinline__ void mfma_chunk_h(f32x16 (&acc)[NT], const float* __restrict__ a_tile, const float* __restrict__ b_row, int lane) {
    const unsigned char* ap = reinterpret_cast<const unsigned char*>(a_tile) + (lane & 31) * 144 + (lane >> 5) * 16;
    const unsigned char* bp = reinterpret_cast<const unsigned char*>(b_row) + (lane >> 5) * 16;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const ak_f16x8 b = *reinterpret_cast<const ak_f16x8*>(bp + 32 * q);
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const ak_f16x8 av = *reinterpret_cast<const ak_f16x8*>(ap + t * 32 * 144 + 32 * q);
            acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(av, b, acc[t], 0, 0, 0);
        }
    }
}

// ------------------------------------------------------------------------------------------------
// anchors x anchors: loss terms (fwd) and dL/dS + dL/d(sums) (bwd), all tables in one pass
// ------------------------------------------------------------------------------------------------
struct AnchorArgs {
    int NT, A, i_lo, i_hi;           // anchor rows [i_lo, i_hi) are this process's shard of block I
    const float* Z[CT_MAXT]; int Dp[CT_MAXT];
    const _Float16* Zh[CT_MAXT];   // optional (MFMA mode 'f16', tables wider than 128 columns): fp16 copy of table k's rows -- its similarities then run
                                   // on v_mfma_f32_32x32x16_f16 (fp16 inputs, fp32 accumulate: the arithmetic of wide16.hip's sweeps)
    const double* sums;            // [NT][8]
    float alpha, kc, ki, itc, iti; // ICL alpha; log2e/tau and 1/tau for ICL (c) and IAL (i)
    double* out;                   // fwd: [NT] icl sums, [M] iala, [M] ialb
    const float* coef;             // bwd: upstream dL/d(out) in the same order
    float* M1[CT_MAXT];            // bwd: stash, M1[k][j*A + i] = dL/dS_k[i,j]
    double* gs;                    // bwd: [NT][8] dL/d(sums)
    const float* SP[CT_MAXT];      // PRE: the similarity blocks formed beforehand (wide16.hip's tile core), SP[k][j * ldp + (i - i_lo)] = X1[i] . X2[j]
    const float* SQ[CT_MAXT];      //      SQ[k][j * ldp + (i - i_lo)] = X2[i] . X1[j]
    long ldp;
};

// PRE: epilogue only -- every table's two similarity blocks are read from memory in the accumulator layout (lanes along i: coalesced), no
// K loop, no LDS tiles (mode 'f16' with all tables wide: the products run on the fp16 tile core at ~0.4 of the fp16 MFMA peak instead of
// this kernel's single-buffered 128 x 64 staging).
template <bool BWD, bool PRE = false>
__global__ __launch_bounds__(CT_THREADS) void anchor_kernel(AnchorArgs a) {
    constexpr int NJT = PRE ? 1 : 2, OT = 32 * NJT;         // (PRE: one 32-column tile per workgroup -- half the live registers of the epilogue)
    constexpr int LR = PRE ? 1 : 128, LO = PRE ? 1 : OT;
    __shared__ __attribute__((aligned(16))) float own1[LR * SGA_LDS_STRIDE];    // X1 rows of block I
    __shared__ __attribute__((aligned(16))) float own2[LR * SGA_LDS_STRIDE];    // X2 rows of block I
    __shared__ __attribute__((aligned(16))) float oth1[LO * SGA_LDS_STRIDE];    // X2 rows of block J  (for P)
    __shared__ __attribute__((aligned(16))) float oth2[LO * SGA_LDS_STRIDE];    // X1 rows of block J  (for Q)
    __shared__ float inv_s[CT_MAXT * 8];                                        // 1/(sum + 1e-9)

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5;
    const int A = a.A, NT = a.NT, M = NT > 1 ? NT - 1 : 0;
    double* const out_s = BWD ? nullptr : a.out + (NT + 2 * M) * (1 + my_slot());
    double* const gs_s = BWD ? a.gs + NT * 8 * (1 + my_slot()) : nullptr;
    for (int e = tid; e < NT * 8; e += CT_THREADS) inv_s[e] = (float)(1.0 / (a.sums[e] + 1e-9));
    const int i0 = a.i_lo + blockIdx.x * 128, j0 = blockIdx.y * OT;
    const int my_i = i0 + wave * 32 + (lane & 31);
    const bool iv = my_i < a.i_hi;
    const int ns = a.i_hi - a.i_lo;

    f32x16 xJ[NJT], gJ[NJT];
    zero_acc<NJT>(xJ);
    zero_acc<NJT>(gJ);

    for (int it = 0; it < NT; ++it) {
        const int k = (NT > 1) ? (it == 0 ? NT - 1 : it - 1) : 0;       // joint first, then the modalities
        const bool is_joint = NT > 1 && it == 0;
        const float* Z = a.Z[k];
        const int Dp = a.Dp[k];
        f32x16 P[NJT], Q[NJT];
        zero_acc<NJT>(P);
        zero_acc<NJT>(Q);
        const _Float16* Zh = a.Zh[k];
        if constexpr (PRE) {
            __syncthreads();                                    // (inv_s)
            const float* sp = a.SP[k] + (iv ? my_i - a.i_lo : 0);
            const float* sq = a.SQ[k] + (iv ? my_i - a.i_lo : 0);
#pragma unroll
            for (int t = 0; t < NJT; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int j = min(j0 + t * 32 + mfma32_row(r, h), A - 1);
                    P[t][r] = sp[(size_t)j * a.ldp];
                    Q[t][r] = sq[(size_t)j * a.ldp];
                }
        } else
        if (Zh) {                                               // uniform: fp16 inputs, 64 columns per chunk
            for (int k0 = 0; k0 < Dp; k0 += 64) {
                __syncthreads();
                lds_load_rows_h<128, CT_THREADS>(own1, Zh, Dp, i0, A, k0, Dp, tid);
                lds_load_rows_h<128, CT_THREADS>(own2, Zh, Dp, A + i0, 2 * A, k0, Dp, tid);
                lds_load_rows_h<OT, CT_THREADS>(oth1, Zh, Dp, A + j0, 2 * A, k0, Dp, tid);
                lds_load_rows_h<OT, CT_THREADS>(oth2, Zh, Dp, j0, A, k0, Dp, tid);
                __syncthreads();
                const int ro = (wave * 32 + (lane & 31)) * SGA_LDS_STRIDE;
                mfma_chunk_h<NJT>(P, oth1, own1 + ro, lane);
                mfma_chunk_h<NJT>(Q, oth2, own2 + ro, lane);
            }
        } else
        for (int k0 = 0; k0 < Dp; k0 += SGA_KC) {
            __syncthreads();
            lds_load_rows<128, CT_THREADS>(own1, Z, Dp, i0, A, k0, Dp, tid);
            lds_load_rows<128, CT_THREADS>(own2, Z, Dp, A + i0, 2 * A, k0, Dp, tid);
            lds_load_rows<OT, CT_THREADS>(oth1, Z, Dp, A + j0, 2 * A, k0, Dp, tid);
            lds_load_rows<OT, CT_THREADS>(oth2, Z, Dp, j0, A, k0, Dp, tid);
            __syncthreads();
            const int ro = (wave * 32 + (lane & 31)) * SGA_LDS_STRIDE;
            mfma_chunk<NJT>(P, oth1, own1 + ro, lane);      // P[i,j] = X1[i].X2[j] = S[i,j]
            mfma_chunk<NJT>(Q, oth2, own2 + ro, lane);      // Q[i,j] = X2[i].X1[j] = S[j,i]
        }
        if (is_joint) {
#pragma unroll
            for (int t = 0; t < NJT; ++t) xJ[t] = P[t];
        }
        const float* is = inv_s + k * 8;                    // [fam*2 + temp]
        const float a11c = is[0], a12c = is[2], a22c = is[4], a21c = is[6];
        const float a11i = is[1], a12i = is[3], a22i = is[5], a21i = is[7];
        const float* js = inv_s + (NT - 1) * 8;
        const float j11 = js[1], j12 = js[3], j22 = js[5], j21 = js[7];

        if (!BWD) {
            float icl = 0.f, la = 0.f, lb = 0.f;
#pragma unroll
            for (int t = 0; t < NJT; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    // (selects, not mask multiplies, here: measured 2 ms faster per launch in this VALU-heavy epilogue)
                    const bool ok = iv && (j0 + t * 32 + mfma32_row(r, h) < A);
                    const float x = P[t][r], y = Q[t][r];
                    const float qa = g_val(fexp2(x * a.kc), a11c, a12c);
                    const float qb = g_val(fexp2(y * a.kc), a22c, a21c);
                    const float term = -flog(a.alpha * qa + (1.f - a.alpha) * qb);
                    icl += ok ? term : 0.f;
                    if (M > 0 && !is_joint) {
                        const float dm = fexp2(x * a.ki), dj = fexp2(xJ[t][r] * a.ki);
                        const float qoa = g_val(dm, a11i, a12i), qma = g_val(dj, j11, j12);
                        const float qob = g_val(dm, a22i, a21i), qmb = g_val(dj, j22, j21);
                        const float ta = __expf(qoa) * (qoa - flog(qma));
                        const float tb = __expf(qob) * (qob - flog(qmb));
                        la += ok ? ta : 0.f;
                        lb += ok ? tb : 0.f;
                    }
                    // one element at a time: fully interleaved, the 32 unrolled elements need >512 registers (spills, 1 wave/SIMD)
                    __builtin_amdgcn_sched_barrier(0);
                }
            icl = wave_sum(icl);
            if (lane == 0) atomicAdd(out_s + k, (double)icl);
            if (M > 0 && !is_joint) {
                la = wave_sum(la);
                lb = wave_sum(lb);
                if (lane == 0) { atomicAdd(out_s + NT + k, (double)la); atomicAdd(out_s + NT + M + k, (double)lb); }
            }
        } else {
            const float c = a.coef[k];
            const float ca = (M > 0 && !is_joint) ? a.coef[NT + k] : 0.f;
            const float cb = (M > 0 && !is_joint) ? a.coef[NT + M + k] : 0.f;
            float gs_c[4] = {0.f, 0.f, 0.f, 0.f};          // this table, ICL temperature
            float gs_i[4] = {0.f, 0.f, 0.f, 0.f};          // this table, IAL temperature
            float gs_j[4] = {0.f, 0.f, 0.f, 0.f};          // joint table, IAL temperature
#pragma unroll
            for (int t = 0; t < NJT; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const bool ok = iv && (j0 + t * 32 + mfma32_row(r, h) < A);
                    const float x = P[t][r], y = Q[t][r];
                    const float dx = fexp2(x * a.kc), dy = fexp2(y * a.kc);
                    const GV Ax = g_full(dx, a11c, a12c), Bx = g_full(dx, a22c, a21c);
                    const float qAy = g_val(dy, a11c, a12c), qBy = g_val(dy, a22c, a21c);
                    const float z_ij = a.alpha * Ax.q + (1.f - a.alpha) * qBy;
                    const float z_ji = a.alpha * qAy + (1.f - a.alpha) * Bx.q;
                    const float wA = ok ? -c * a.alpha * frcp(z_ij) : 0.f;
                    const float wB = ok ? -c * (1.f - a.alpha) * frcp(z_ji) : 0.f;
                    float gx = (wA * Ax.dd + wB * Bx.dd) * dx * a.itc;
                    gs_c[0] += wA * Ax.dsa; gs_c[1] += wA * Ax.dsb; gs_c[2] += wB * Bx.dsa; gs_c[3] += wB * Bx.dsb;
                    if (M > 0 && !is_joint) {
                        const float dm = fexp2(x * a.ki), dj = fexp2(xJ[t][r] * a.ki);
                        const GV OA = g_full(dm, a11i, a12i), OB = g_full(dm, a22i, a21i);
                        const GV MA = g_full(dj, j11, j12), MB = g_full(dj, j22, j21);
                        const float eA = ok ? __expf(OA.q) : 0.f, eB = ok ? __expf(OB.q) : 0.f;
                        const float tA = ca * eA * (OA.q - flog(MA.q) + 1.f), uA = -ca * eA * frcp(MA.q);
                        const float tB = cb * eB * (OB.q - flog(MB.q) + 1.f), uB = -cb * eB * frcp(MB.q);
                        gx += (tA * OA.dd + tB * OB.dd) * dm * a.iti;
                        gJ[t][r] += (uA * MA.dd + uB * MB.dd) * dj * a.iti;
                        gs_i[0] += tA * OA.dsa; gs_i[1] += tA * OA.dsb; gs_i[2] += tB * OB.dsa; gs_i[3] += tB * OB.dsb;
                        gs_j[0] += uA * MA.dsa; gs_j[1] += uA * MA.dsb; gs_j[2] += uB * MB.dsa; gs_j[3] += uB * MB.dsb;
                    }
                    P[t][r] = gx;
                    __builtin_amdgcn_sched_barrier(0);
                }
#pragma unroll
            for (int f = 0; f < 4; ++f) {
                const float vc = wave_sum(gs_c[f]);
                if (lane == 0 && vc != 0.f) atomicAdd(gs_s + k * 8 + f * 2 + 0, (double)vc);
                if (M > 0 && !is_joint) {
                    const float vi = wave_sum(gs_i[f]), vj = wave_sum(gs_j[f]);
                    if (lane == 0 && vi != 0.f) atomicAdd(gs_s + k * 8 + f * 2 + 1, (double)vi);
                    if (lane == 0 && vj != 0.f) atomicAdd(gs_s + (NT - 1) * 8 + f * 2 + 1, (double)vj);
                }
            }
            if (is_joint) {
#pragma unroll
                for (int t = 0; t < NJT; ++t) gJ[t] = P[t];
            } else if (iv) {
                float* m1 = a.M1[k];
#pragma unroll
                for (int t = 0; t < NJT; ++t)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int j = j0 + t * 32 + mfma32_row(r, h);
                        if (j < A) m1[(size_t)j * ns + (my_i - a.i_lo)] = P[t][r];
                    }
            }
        }
    }
    if (BWD && NT > 1 && iv) {
        float* m1 = a.M1[NT - 1];
#pragma unroll
        for (int t = 0; t < NJT; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int j = j0 + t * 32 + mfma32_row(r, h);
                if (j < A) m1[(size_t)j * ns + (my_i - a.i_lo)] = gJ[t][r];
            }
    }
}

// ------------------------------------------------------------------------------------------------
// dZ anchor rows from the dL/dS stash (M1[j*A + i] = dL/dS[i,j]) without LDS:
//   TRANS = 1 :  dX1[i, :] += sum_j M1[j, i] X2[j, :]      (A operand column-read: coalesced along i)
//   TRANS = 0 :  dX2[j, :] += sum_i M1[j, i] X1[i, :]      (A operand row-read: float4 along i)
// One wave owns a 32-row output block and NCT 32-column tiles; both MFMA operands are loaded straight from
// global/L2 in fragment order (the B rows X[k, :] are shared by every wave and stay L2/L1 resident), K is split
// across blockIdx.y and the partial tiles are added atomically into the zero-initialised dZ rows.
// ------------------------------------------------------------------------------------------------
template <int NCT, bool TRANS>
__global__ __launch_bounds__(256) void stash_gemm_kernel(const float* __restrict__ M1, const float* __restrict__ X,
                                                         float* __restrict__ out, int MR, int KR, int ldm, int ld, int Dp, int k_per_split) {
    // out[MR rows] += op(M1)[MR, KR] X[KR rows];  op(M1)[m,k] = TRANS ? M1[k*ldm + m] : M1[m*ldm + k].
    // X / out point at the first column of this launch's column block; rows are `ld` floats apart, Dp columns are valid
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, h = lane >> 5, l31 = lane & 31;
    const int m0 = (blockIdx.x * 4 + wave) * 32;
    if (m0 >= MR) return;
    const int kbeg = blockIdx.y * k_per_split, kend = min(KR, kbeg + k_per_split);
    const int m = min(m0 + l31, MR - 1);                // clamped rows are computed but never stored
    f32x16 acc[NCT];
    zero_acc<NCT>(acc);
    int ncol[NCT];
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct) ncol[ct] = min(ct * 32 + l31, Dp - 1);
    for (int k0 = kbeg; k0 < kend; k0 += 8) {           // A, k_per_split multiples of 8 are not required: tail clamps + masks
        float av[4];
        float kmask[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int k = k0 + 4 * h + r;
            kmask[r] = k < kend ? 1.f : 0.f;
            const int kc = min(k, KR - 1);
            av[r] = (TRANS ? M1[(size_t)kc * ldm + m] : M1[(size_t)m * ldm + kc]) * kmask[r];
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int kc = min(k0 + 4 * h + r, KR - 1);
            const float* xr = X + (size_t)kc * ld;
#pragma unroll
            for (int ct = 0; ct < NCT; ++ct) acc[ct] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[r], xr[ncol[ct]], acc[ct], 0, 0, 0);
        }
    }
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct) {
        const int d = ct * 32 + l31;
        if (d < Dp) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = m0 + mfma32_row(r, h);
                if (row < MR) atomicAdd(out + (size_t)row * ld + d, acc[ct][r]);
            }
        }
    }
}
}  // namespace

static int total_blocks(const SweepArgs& a) {
    int n = 0;
    for (int g = 0; g < a.ngroups; ++g) n += (a.grp[g].nown + 127) / 128;
    return n;
}

extern "C" int sga_loss_neg_sums(const float* Z, int Dp, int A, int J1, int J2, float tau0, float tau1, double* sums8,
                                 void* stream) {
    return sga_loss_neg_sums_shard(Z, Dp, A, J1, J2, tau0, tau1, sums8, 0, A, stream);
}

extern "C" int sga_loss_neg_sums_shard(const float* Z, int Dp, int A, int J1, int J2, float tau0, float tau1, double* sums8,
                                       int a_lo, int a_hi, void* stream) {
    SGA_CHECK_ARG(Z && sums8 && Dp % 8 == 0 && A >= 0 && J1 >= 0 && J2 >= 0 && tau0 > 0 && tau1 > 0, "sga_loss_neg_sums: bad argument");
    SGA_CHECK_ARG(a_lo >= 0 && a_lo <= a_hi && a_hi <= A, "sga_loss_neg_sums: anchor shard [%d,%d) outside [0,%d]", a_lo, a_hi, A);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (int rc = zero_slots(sums8, 8, s, "sga_loss_neg_sums")) return rc;
    if (A == 0 || a_hi == a_lo || (J1 == 0 && J2 == 0)) return SGA_OK;
    SweepArgs a{};
    a.Z = Z; a.Dp = Dp; a.k0 = LOG2E / tau0; a.k1 = LOG2E / tau1; a.it0 = 1.f / tau0; a.it1 = 1.f / tau1;
    a.sums = sums8; a.gs = nullptr; a.dZ = nullptr; a.col0 = 0;
    a.ngroups = fill_groups(a.grp, A, J1, J2, false, a_lo, a_hi);
    const int nblk = total_blocks(a);
    const int jt = ((J1 > J2 ? J1 : J2) + 127) / 128;
    int gy = (8 * sga_num_cus() + nblk - 1) / nblk;
    if (gy > jt) gy = jt;
    if (gy < 1) gy = 1;
    if (Dp == 104) launch_sweep_fast<13, false>(a, nblk, gy, s);
    else if (Dp == 128) launch_sweep_fast<16, false>(a, nblk, gy, s);
    else launch_sweep<4, 1, false>(a, nblk, gy, s);
    fold_slots(sums8, 8, s);
    SGA_CHECK_LAUNCH("sga_loss_neg_sums");
    return SGA_OK;
}

extern "C" int sga_loss_neg_grad(const float* Z, int Dp, int A, int J1, int J2, float tau0, float tau1,
                                 const double* gs8, float* dZ, void* stream) {
    return sga_loss_neg_grad_shard(Z, Dp, A, J1, J2, tau0, tau1, gs8, dZ, 0, A, stream);
}

extern "C" int sga_loss_neg_grad_shard(const float* Z, int Dp, int A, int J1, int J2, float tau0, float tau1,
                                       const double* gs8, float* dZ, int a_lo, int a_hi, void* stream) {
    SGA_CHECK_ARG(Z && gs8 && dZ && Dp % 8 == 0 && A >= 0 && J1 >= 0 && J2 >= 0, "sga_loss_neg_grad: bad argument");
    SGA_CHECK_ARG(a_lo >= 0 && a_lo <= a_hi && a_hi <= A, "sga_loss_neg_grad: anchor shard [%d,%d) outside [0,%d]", a_lo, a_hi, A);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (A == 0 || a_hi == a_lo || (J1 == 0 && J2 == 0)) return SGA_OK;
    SweepArgs a{};
    a.Z = Z; a.Dp = Dp; a.k0 = LOG2E / tau0; a.k1 = LOG2E / tau1; a.it0 = 1.f / tau0; a.it1 = 1.f / tau1;
    a.sums = nullptr; a.gs = gs8; a.dZ = dZ;
    a.ngroups = fill_groups(a.grp, A, J1, J2, true, a_lo, a_hi);
    const int nblk = total_blocks(a);
    int mx = A > J1 ? A : J1;
    if (J2 > mx) mx = J2;
    int gy = (6 * sga_num_cus() + nblk - 1) / nblk;
    if (Dp <= 128) {
        const int jt = (mx + 127) / 128;
        if (gy > jt) gy = jt;
        if (gy < 1) gy = 1;
        a.col0 = 0;
        if (Dp == 104) launch_sweep_fast<13, true>(a, nblk, gy, s);
        else if (Dp == 128) launch_sweep_fast<16, true>(a, nblk, gy, s);
        else launch_sweep<4, 4, true>(a, nblk, gy, s);
    } else {
        const int jt = (mx + 63) / 64;
        if (gy > jt) gy = jt;
        if (gy < 1) gy = 1;
        for (int col0 = 0; col0 < Dp; col0 += 320) {       // 10 column tiles per pass: one pass for the 300-d joint table
            a.col0 = col0;
            launch_sweep<2, 10, true>(a, nblk, gy, s);
        }
    }
    SGA_CHECK_LAUNCH("sga_loss_neg_grad");
    return SGA_OK;
}

extern "C" size_t sga_loss_neg_grad_wide_floats(int A, int J1, int J2) {
    return (size_t)2 * (size_t)(J1 + J2) * (size_t)((A + 31) / 32 * 32);       // the whole batch in one block; less is allowed
}

extern "C" int sga_loss_neg_grad_wide(const float* Z, int Dp, int A, int J1, int J2, float tau0, float tau1, const double* gs8,
                                      float* dZ, float* stash, size_t stash_floats, void* stream) {
    SGA_CHECK_ARG(Z && gs8 && dZ && stash && Dp % 8 == 0 && A >= 0 && J1 >= 0 && J2 >= 0, "sga_loss_neg_grad_wide: bad argument");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int J = J1 + J2;
    if (A == 0 || J == 0) return SGA_OK;
    size_t rows = stash_floats / ((size_t)2 * J);
    if (rows >= (size_t)A) rows = A; else rows = rows / 32 * 32;
    SGA_CHECK_ARG(rows >= 32 || rows == (size_t)A, "sga_loss_neg_grad_wide: workspace holds fewer than 32 anchor rows (%zu floats for J = %d)", stash_floats, J);
    const int n1 = 2 * A, n2 = 2 * A + J1;
    for (int lo = 0; lo < A; lo += (int)rows) {
        const int hi = lo + (int)rows < A ? lo + (int)rows : A, ns = hi - lo;
        CoefArgs a{};
        a.Z = Z; a.Dp = Dp; a.k0 = LOG2E / tau0; a.k1 = LOG2E / tau1; a.it0 = 1.f / tau0; a.it1 = 1.f / tau1; a.gs = gs8;
        a.ld = ns; a.n1 = n1;
        a.stash[0] = stash; a.stash[1] = stash + (size_t)J * ns;
        const int nb = (ns + 127) / 128;
        a.grp[0] = SweepGroup{lo, ns, 0, 2, {SweepSeg{n1, J1, 0}, SweepSeg{n2, J2, 1}}, 1};            // X1 anchors: s11, s12
        a.grp[1] = SweepGroup{A + lo, ns, nb, 2, {SweepSeg{n2, J2, 2}, SweepSeg{n1, J1, 3}}, 1};       // X2 anchors: s22, s21
        const int mx = J1 > J2 ? J1 : J2;
        int gy = (6 * sga_num_cus() + 2 * nb - 1) / (2 * nb);
        const int jt = (mx + 63) / 64;
        if (gy > jt) gy = jt;
        if (gy < 1) gy = 1;
        hipLaunchKernelGGL(sweep_coef_kernel<2>, dim3(2 * nb, gy), dim3(CT_THREADS), 0, s, a);
        SGA_CHECK_LAUNCH("sga_loss_neg_grad_wide");
        for (int g = 0; g < 2; ++g) {
            const float* C = a.stash[g];
            const size_t own_row = (size_t)(g == 0 ? lo : A + lo);
            // dZ[anchors of the block] += Ct^T Z[negatives]
            int rc = sga_gemm(1, 0, ns, Dp, J, C, ns, 0, Z + (size_t)n1 * Dp, Dp, dZ + own_row * Dp, Dp, nullptr, 1, stream);
            if (rc) return rc;
            // dZ[negatives] += Ct Z[anchors of the block]
            rc = sga_gemm(0, 0, J, Dp, ns, C, ns, 0, Z + own_row * Dp, Dp, dZ + (size_t)n1 * Dp, Dp, nullptr, 1, stream);
            if (rc) return rc;
        }
    }
    return SGA_OK;
}

static int fill_anchor(AnchorArgs& a, const float* const* Z, const int* Dp, int NT, int A, const double* sums,
                       float alpha, float tau_icl, float tau_ial, int a_lo, int a_hi) {
    if (NT < 1 || NT > CT_MAXT) { sga_set_error("sga_loss_anchor: NT=%d outside [1,%d]", NT, CT_MAXT); return SGA_ERR_ARG; }
    if (a_lo < 0 || a_hi > A || a_lo > a_hi) { sga_set_error("sga_loss_anchor: anchor shard [%d,%d) outside [0,%d]", a_lo, a_hi, A); return SGA_ERR_ARG; }
    a.NT = NT; a.A = A; a.sums = sums; a.alpha = alpha; a.i_lo = a_lo; a.i_hi = a_hi;
    a.kc = LOG2E / tau_icl; a.ki = LOG2E / tau_ial; a.itc = 1.f / tau_icl; a.iti = 1.f / tau_ial;
    for (int k = 0; k < NT; ++k) {
        if (!Z[k] || Dp[k] % 8) { sga_set_error("sga_loss_anchor: table %d null or Dp %% 8 != 0", k); return SGA_ERR_ARG; }
        a.Z[k] = Z[k]; a.Dp[k] = Dp[k];
    }
    return SGA_OK;
}

// A workspace given (the caller's choice: wide tables): the 2 NT similarity blocks of the anchor shard are formed first -- tables with an
// fp16 copy Zh[k] on wide16.hip's fp16 tile core (up to 8 blocks per launch), the others by the exact-fp32 NT GEMM of gemm.hip -- and the
// epilogue-only form of the kernel reads them.
static size_t anchor_ws_ldp(int ns) { return (size_t)(ns + 3) / 4 * 4; }
extern "C" size_t sga_loss_anchor_f16_ws_bytes(int NT, int A, int ns) {
    if (NT < 1 || A < 1 || ns < 1) return 256;
    return (size_t)NT * 2 * A * anchor_ws_ldp(ns) * sizeof(float) + 256;
}
static int anchor_pre_blocks(AnchorArgs& a, const void* const* Zh, void* ws, size_t ws_bytes, hipStream_t s, bool& pre) {
    pre = false;
    if (!ws) return SGA_OK;
    const int ns = a.i_hi - a.i_lo, A = a.A;
    if (ws_bytes < sga_loss_anchor_f16_ws_bytes(a.NT, A, ns)) {
        sga_set_error("sga_loss_anchor (f16): workspace of %zu bytes, %zu needed", ws_bytes, sga_loss_anchor_f16_ws_bytes(a.NT, A, ns));
        return SGA_ERR_WORKSPACE;
    }
    const size_t ldp = anchor_ws_ldp(ns);
    float* w = static_cast<float*>(ws);
    SgaW16Store e[8];
    int n = 0;
    for (int k = 0; k < a.NT; ++k) {
        const _Float16* zh = Zh ? static_cast<const _Float16*>(Zh[k]) : nullptr;
        const long dp = a.Dp[k];
        float* sp = w + (size_t)(2 * k) * A * ldp;
        float* sq = w + (size_t)(2 * k + 1) * A * ldp;
        a.SP[k] = sp; a.SQ[k] = sq;
        if (zh) {
            e[n++] = SgaW16Store{zh + (size_t)A * dp, dp, A, zh + (size_t)a.i_lo * dp, dp, ns, (int)dp, sp, (long)ldp};      // X2[j] . X1[i]
            e[n++] = SgaW16Store{zh, dp, A, zh + (size_t)(A + a.i_lo) * dp, dp, ns, (int)dp, sq, (long)ldp};                  // X1[j] . X2[i]
        } else {
            const float* z = a.Z[k];
            if (int rc = sga_gemm(0, 1, A, ns, (int)dp, z + (size_t)A * dp, dp, 0, z + (size_t)a.i_lo * dp, dp, sp, (long)ldp, nullptr, 0, s)) return rc;
            if (int rc = sga_gemm(0, 1, A, ns, (int)dp, z, dp, 0, z + (size_t)(A + a.i_lo) * dp, dp, sq, (long)ldp, nullptr, 0, s)) return rc;
        }
        if (n == 8 || (k == a.NT - 1 && n > 0)) {
            if (int rc = sga_wide16_store_batch(e, n, s)) return rc;
            n = 0;
        }
    }
    a.ldp = (long)ldp;
    pre = true;
    return SGA_OK;
}

extern "C" int sga_loss_anchor_fwd_f16(const float* const* Z, const void* const* Zh, const int* Dp, int NT, int A, const double* sums,
                                       float alpha, float tau_icl, float tau_ial, double* out, int a_lo, int a_hi, void* ws, size_t ws_bytes,
                                       void* stream) {
    SGA_CHECK_ARG(Z && Dp && sums && out && A >= 0, "sga_loss_anchor_fwd_f16: bad argument");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int M = NT > 1 ? NT - 1 : 0;
    if (int rc0 = zero_slots(out, NT + 2 * M, s, "sga_loss_anchor_fwd_f16")) return rc0;
    if (A == 0 || a_hi <= a_lo) return SGA_OK;
    AnchorArgs a{};
    int rc = fill_anchor(a, Z, Dp, NT, A, sums, alpha, tau_icl, tau_ial, a_lo, a_hi);
    if (rc) return rc;
    a.out = out;
    for (int k = 0; k < NT; ++k) a.Zh[k] = Zh ? static_cast<const _Float16*>(Zh[k]) : nullptr;
    bool pre = false;
    if (int rcp = anchor_pre_blocks(a, Zh, ws, ws_bytes, s, pre)) return rcp;
    if (pre) hipLaunchKernelGGL((anchor_kernel<false, true>), dim3((a_hi - a_lo + 127) / 128, (A + 31) / 32), dim3(CT_THREADS), 0, s, a);
    else hipLaunchKernelGGL(anchor_kernel<false>, dim3((a_hi - a_lo + 127) / 128, (A + 63) / 64), dim3(CT_THREADS), 0, s, a);
    fold_slots(out, NT + 2 * M, s);
    SGA_CHECK_LAUNCH("sga_loss_anchor_fwd_f16");
    return SGA_OK;
}

extern "C" int sga_loss_anchor_bwd_f16(const float* const* Z, const void* const* Zh, const int* Dp, int NT, int A, const double* sums,
                                       float alpha, float tau_icl, float tau_ial, const float* coef, float* const* M1,
                                       double* gs, int a_lo, int a_hi, void* ws, size_t ws_bytes, void* stream) {
    SGA_CHECK_ARG(Z && Dp && sums && coef && M1 && gs && A >= 0, "sga_loss_anchor_bwd_f16: bad argument");
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (int rc0 = zero_slots(gs, NT * 8, s, "sga_loss_anchor_bwd_f16")) return rc0;
    if (A == 0 || a_hi <= a_lo) return SGA_OK;
    AnchorArgs a{};
    int rc = fill_anchor(a, Z, Dp, NT, A, sums, alpha, tau_icl, tau_ial, a_lo, a_hi);
    if (rc) return rc;
    a.coef = coef; a.gs = gs;
    for (int k = 0; k < NT; ++k) { SGA_CHECK_ARG(M1[k], "sga_loss_anchor_bwd_f16: null stash %d", k); a.M1[k] = M1[k]; }
    for (int k = 0; k < NT; ++k) a.Zh[k] = Zh ? static_cast<const _Float16*>(Zh[k]) : nullptr;
    bool pre = false;
    if (int rcp = anchor_pre_blocks(a, Zh, ws, ws_bytes, s, pre)) return rcp;
    if (pre) hipLaunchKernelGGL((anchor_kernel<true, true>), dim3((a_hi - a_lo + 127) / 128, (A + 31) / 32), dim3(CT_THREADS), 0, s, a);
    else hipLaunchKernelGGL(anchor_kernel<true>, dim3((a_hi - a_lo + 127) / 128, (A + 63) / 64), dim3(CT_THREADS), 0, s, a);
    fold_slots(gs, NT * 8, s);
    SGA_CHECK_LAUNCH("sga_loss_anchor_bwd_f16");
    return SGA_OK;
}

/* For one table (Z = [X1 | X2 | ...] rows of width Dp) and the anchor shard [a_lo, a_hi) that produced M1 [A, a_hi-a_lo]:
 * dZ[a_lo:a_hi] += M1^T X2   and   dZ[A:2A] += M1 X1[a_lo:a_hi] */
static void launch_stash(bool trans, int nct10, const float* M1, const float* X, float* out, int MR, int KR, int ldm, int ld,
                         int w, hipStream_t s) {
    const int gx = (MR + 127) / 128;
    int splits = (6 * sga_num_cus() + gx - 1) / gx;
    int kper = ((KR + splits - 1) / splits + 7) / 8 * 8;
    if (kper < 64) kper = 64;
    splits = (KR + kper - 1) / kper;
    dim3 grid(gx, splits), blk(256);
    if (trans) {
        if (nct10) hipLaunchKernelGGL((stash_gemm_kernel<10, true>), grid, blk, 0, s, M1, X, out, MR, KR, ldm, ld, w, kper);
        else hipLaunchKernelGGL((stash_gemm_kernel<4, true>), grid, blk, 0, s, M1, X, out, MR, KR, ldm, ld, w, kper);
    } else {
        if (nct10) hipLaunchKernelGGL((stash_gemm_kernel<10, false>), grid, blk, 0, s, M1, X, out, MR, KR, ldm, ld, w, kper);
        else hipLaunchKernelGGL((stash_gemm_kernel<4, false>), grid, blk, 0, s, M1, X, out, MR, KR, ldm, ld, w, kper);
    }
}

extern "C" int sga_loss_stash_grad(const float* M1, const float* Z, int A, int Dp, float* dZ, int a_lo, int a_hi, void* stream) {
    SGA_CHECK_ARG(M1 && Z && dZ && A >= 0 && Dp >= 8 && Dp % 8 == 0 && a_lo >= 0 && a_hi <= A && a_lo <= a_hi, "sga_loss_stash_grad: bad argument");
    const int ns = a_hi - a_lo;
    if (A == 0 || ns == 0) return SGA_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const float* X1 = Z + (size_t)a_lo * Dp;             // the shard's X1 rows
    const float* X2 = Z + (size_t)A * Dp;                // all X2 rows
    if (ns % 4 == 0 && Dp % 4 == 0 && reinterpret_cast<uintptr_t>(M1) % 16 == 0 && reinterpret_cast<uintptr_t>(Z) % 16 == 0 &&
        reinterpret_cast<uintptr_t>(dZ) % 16 == 0) {
        // the two products as plain GEMMs on the stash M1 [A (j), ns (i)] = G^T (gemm.hip: row-major TN / NN kernels,
        // split over the contraction with atomic accumulation into dZ):
        //   dX1[i, :] += sum_j M1[j, i] X2[j, :]      (TN)          dX2[j, :] += sum_i M1[j, i] X1[i, :]      (NN)
        int rc = sga_gemm(1, 0, ns, Dp, A, M1, ns, 0, X2, Dp, dZ + (size_t)a_lo * Dp, Dp, nullptr, 1, stream);
        if (rc) return rc;
        return sga_gemm(0, 0, A, Dp, ns, M1, ns, 0, X1, Dp, dZ + (size_t)A * Dp, Dp, nullptr, 1, stream);
    }
    for (int c0 = 0; c0 < Dp; c0 += 320) {               // column blocks of <= 320
        const int w = Dp - c0 < 320 ? Dp - c0 : 320;
        launch_stash(true, w > 128, M1, X2 + c0, dZ + (size_t)a_lo * Dp + c0, ns, A, ns, Dp, w, s);
        launch_stash(false, w > 128, M1, X1 + c0, dZ + (size_t)A * Dp + c0, A, ns, ns, Dp, w, s);
    }
    SGA_CHECK_LAUNCH("sga_loss_stash_grad");
    return SGA_OK;
}
