// Dense node-similarity + contrastive (ICL) / alignment (IAL) loss, forward and backward, without
// ever materialising an anchors x negatives matrix.
//
// Replaces reference src/aligner/losses.py: calculate_prob_dist :5-15, ICLLoss.forward :43-58,
// IALLoss.forward :68-97 (and their autograd).  For each embedding table k (modalities + 'joint')
// with L2-normalised rows and index sets e1i/e2i (A anchors each), e1j (J1), e2j (J2):
//     X1 = E[e1i], X2 = E[e2i], N1 = E[e1j], N2 = E[e2j]            (packed row blocks of Z_k)
//     s11 = sum exp(X1 N1^T/t)  s12 = sum exp(X1 N2^T/t)  s22 = sum exp(X2 N2^T/t)  s21 = sum exp(X2 N1^T/t)
//     S = X1 X2^T ;  qA[i,j] = g(exp(S[i,j]/t); s11, s12) ;  qB[i,j] = g(exp(S[j,i]/t); s22, s21)
//     g(d; sa, sb) = 1 / (1 + 1/(d/(sa+1e-9)+1e-9) + 1/(d/(sb+1e-9)+1e-9) + 1e-9)
//     ICL_k  = sum_ij -log(a qA + (1-a) qB)                         (t = 0.1; the mean's 1/A^2 is applied by the host)
//     IALa_m = sum_ij exp(qoA)(qoA - log qmA), IALb_m likewise with qB   (t = 1; qo from table m, qm from 'joint')
//
// Kernel set (all exact fp32 on v_mfma_f32_32x32x2_f32, fp64 only for the global scalar sums):
//   gather      E, idx            -> Z (normalised, K padded to a multiple of 8), row norms
//   sweep<sum>  Z                 -> the 4x2 global sums per table           (anchors x negatives, pass 1)
//   anchor<fwd> Z (all tables)    -> ICL / IALa / IALb sums                  (anchors x anchors,  pass 2)
//   anchor<bwd> Z, upstream coefs -> dL/dS stash (transposed) + dL/d(sums)   (anchors x anchors)
//   (sga_gemm)  stash, Z          -> dZ anchor rows
//   sweep<grad> Z, dL/d(sums)     -> dZ += coefficient-weighted negatives    (owner-stationary, two sweeps)
//   scatter     dZ, Z, norms, idx -> dE (normalisation Jacobian + index_add)
// S tiles are produced in the orientation "lane = owner row, registers = other rows", which is also
// the MFMA A-operand layout, so the gradient GEMM (coefficients x other rows) chains straight from the
// accumulators with no LDS transpose and each owner row is accumulated by exactly one wave.
// This file: gather / scatter and the fused fp32 sweeps.  The per-table kernels are in loss_pertable.hip, the fused anchors x anchors
// kernels in loss_anchor.hip; sweep_groups.h holds the row-group plan the sweeps share.
#include "mfma_tiles.h"
#include <type_traits>

#include "loss_math.h"
#include "sweep_groups.h"

namespace {

// ------------------------------------------------------------------------------------------------
// gather + normalise:  Z[r, :] = E[idx[r], :] / max(||.||, 1e-12), zero padded to Dp; nrm[r] = ||.||
// (F.normalize(emb, dim=1) then emb[data_dict[...]]: losses.py:44-48, :73-79, :84-87)
// ------------------------------------------------------------------------------------------------
__global__ void gather_normalize_kernel(const float* __restrict__ E, int D, const int* __restrict__ idx, int R,
                                        float* __restrict__ Z, int Dp, float* __restrict__ nrm) {
    const int lane = threadIdx.x & 63, wpb = blockDim.x >> 6;
    for (int r = blockIdx.x * wpb + (threadIdx.x >> 6); r < R; r += gridDim.x * wpb) {
        const float* x = E + (size_t)idx[r] * D;
        float ss = 0.f;
        for (int d = lane; d < D; d += 64) { const float v = x[d]; ss += v * v; }
        ss = wave_sum(ss);
        const float n = sqrtf(ss);
        const float inv = 1.f / fmaxf(n, 1e-12f);
        float* z = Z + (size_t)r * Dp;
        for (int d = lane; d < Dp; d += 64) z[d] = d < D ? x[d] * inv : 0.f;
        if (lane == 0) nrm[r] = n;
    }
}

// dE[idx[r], :] += J_normalize^T dZ[r, :]
__global__ void scatter_normalize_bwd_kernel(const float* __restrict__ dZ, const float* __restrict__ Z,
                                             const float* __restrict__ nrm, const int* __restrict__ idx, int R, int D,
                                             int Dp, float* __restrict__ dE) {
    const int lane = threadIdx.x & 63, wpb = blockDim.x >> 6;
    for (int r = blockIdx.x * wpb + (threadIdx.x >> 6); r < R; r += gridDim.x * wpb) {
        const float* g = dZ + (size_t)r * Dp;
        const float* z = Z + (size_t)r * Dp;
        float dot = 0.f;
        for (int d = lane; d < D; d += 64) dot += g[d] * z[d];
        dot = wave_sum(dot);
        const float n = nrm[r];
        const bool clamped = n < 1e-12f;
        const float inv = 1.f / fmaxf(n, 1e-12f);
        if (clamped) dot = 0.f;
        float* o = dE + (size_t)idx[r] * D;
        for (int d = lane; d < D; d += 64) atomicAdd(o + d, (g[d] - z[d] * dot) * inv);
    }
}

// ------------------------------------------------------------------------------------------------
// Fused multi-table sweeps ("joint = fusion of these tables" case, the normal pipeline).
//
// The joint row is cat_m(w_m zhat_m)/||.|| (sg_aligner.py:32-34 followed by F.normalize in losses.py:44,
// 73), so with beta_m = w_m^2 / sum_k w_k^2 every joint similarity is  S_J = sum_m beta_m S_m : the 300-d
// table never has to be multiplied.  One launch computes the M modality S tiles of an
// (owner block, other tile) pair, derives S_J, and
//   SUM  mode: accumulates the 4x2 global sums of all M+1 tables;
//   GRAD mode: forms c_m = dL/dS_m + beta_m dL/dS_J, chains the M gradient GEMMs from the accumulators,
//              and accumulates Gamma_m = sum dL/dS_J * S_m  (= dL/dbeta_m through the negatives).
// vs. the per-table path this removes the joint table's S and gradient GEMMs (~half of all loss FLOPs).
// 32-row other tiles for all M tables are streamed into a double-buffered LDS ring by global_load_lds DMA (no VGPR
// round trip) one step ahead of the MFMAs.  Requires Dp == 104 (emb_dim 100) and 32 readable rows past the end of
// every Z buffer.  (A 32x32x2 form of this kernel -- 32 owner rows per wave, the whole 512-entry register file, one
// wave per SIMD -- ran the gradient sweep in 22.5 ms; sweep16_kernel below replaced it at 19.4 ms.)
// ------------------------------------------------------------------------------------------------
struct MultiArgs {
    int M; const float* Z[4]; int ngroups; SweepGroup grp[4];
    float k0, k1, it0, it1;
    const float* beta;              // [M]
    double* sums;                   // [(M+1)][8]            SUM out
    const double* gs;               // [(M+1)][8]            GRAD in (joint = row M)
    float* dZ[4];                   // GRAD out, atomic accumulate
    double* gamma;                  // [M]                   GRAD out
    int ktail;                      // K steps of 4 past k = 96 that hold data: ceil((D - 96) / 4), D = 100 -> 1 (columns 100..103 are zero padding)
    int swap_tail;                  // centred tables (sga_loss_centre_tables: columns 100 = b, 101 = 1): the OWNER reads columns 100 and 101 swapped, so that the K tail adds b_i + b_j
};

// ------------------------------------------------------------------------------------------------
// 16x16x4 form of the fused multi-table sweep (M = 2, 3; the path the benchmark runs).
//
// The 32x32 predecessor kept M*52 owner-operand registers and M*64 gradient accumulators per lane: the whole
// 512-entry file, one wave per SIMD, so nothing overlaps its exp2/coefficient VALU work with MFMA (measured 70 % of
// the fp32 MFMA peak).  Here a wave owns 16 rows instead of 32: M*26 operand + M*28 accumulator registers, 8 waves
// per workgroup = two per SIMD, and the second wave's MFMAs run under the first one's epilogue.  Same workgroup
// geometry otherwise (128 owner rows, 32-row other tiles of all M tables through the double-buffered DMA ring), so
// plan_multi's uniform work units are shared.  The gradient GEMM is 7 column tiles of 16 (112 >= 104) instead of
// 4 of 32 (128): 12 % less padded MFMA work.
//
// MFMA bookkeeping (v_mfma_f32_16x16x4_f32: A lane&15 = row, B lane&15 = column, lane>>4 = k; D[4*(lane>>4)+r][lane&15]):
//   S^T tile:  A = other rows from LDS, B = owner rows (registers)  ->  lane&15 = owner row, (lane>>4, r) = other row
//   which is exactly the A-operand layout of  dZ[own, :] += C[own, other] * Z[other, :]  with k = lane>>4.
// D row rho = 4*(lane>>4) + r holds other row pi(rho) = rho with bits 1 and 2 swapped: the gradient GEMM's B reads
// (ds_read_b32, lanes 0-31 = two k groups) then hit rows 2 apart = 16 banks apart instead of the same 16 banks.
// ------------------------------------------------------------------------------------------------
constexpr int S16_WAVES = 4;   // waves per workgroup; with 4, two workgroups share a CU (2 x 78 KiB of LDS)
// The owner rows (the S product's register operand, used for nothing else) carry the factor log2(e)/tau1, so the MFMA result is
// already the exp2 argument of the tau1 terms and the tau0 argument is one multiply away (k0/k1).  (Round 3; also tried there and
// dropped: gradient columns 96..99 on VALU -- a broadcast ds_read_b128 + 4 FMAs per step instead of the 7th, 3/4-padded MFMA
// tile: 24 MFMAs per tile less, same time; tools/experiments/r03_sweep16_vtail_prescale_nomask.diff.txt.)
constexpr int S16_THREADS = S16_WAVES * 64;
constexpr int S16_OWN = S16_WAVES * 16;     // owner rows per workgroup
// (profiles/HISTORY.md lists what the timing-only ablations of this kernel -- no barrier, DMA, exp2, S product, gradient GEMM -- measured.)
__device__ __forceinline__ int s16_pi(int rho) { return (rho & 9) | ((rho & 2) << 1) | ((rho & 4) >> 1); }
// A wave-uniform float that was produced by VALU arithmetic (so it sits in a VGPR) moved to an SGPR.
__device__ __forceinline__ float to_sgpr(float x) { return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, x))); }

// KT2: the table is wider than 100 columns (a second K step past k = 96 holds data).  emb_dim = 100 runs the KT2 = false build, whose
// register file has no room for the 2 M operands of a step it would never execute.
template <int M, bool GRAD, bool KT2 = false>
__global__ __launch_bounds__(S16_THREADS, M <= 3 ? 2 : 1) void sweep16_kernel(MultiArgs a) {
    constexpr int DP = 104, OT = 32, NCT = 7, NTL = KT2 ? 2 : 1;
    constexpr int TILE_F = OT * DP, BUF_F = M * TILE_F;
    extern __shared__ __attribute__((aligned(16))) float lds[];     // [2][M][OT][DP] + slack for the 7th column tile

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g4 = lane >> 4, l15 = lane & 15;
    int g = 0;
#pragma unroll
    for (int i = 1; i < 4; ++i) if (i < a.ngroups && (int)blockIdx.x >= a.grp[i].blk0) g = i;
    const SweepGroup& grp = a.grp[g];
    // XCD-aware work order.  Workgroup b is dispatched to XCD b % 8 (its own 4 MiB L2); a group's work list, ordered (split major,
    // owner block minor), is cut into 8 contiguous chunks, one per XCD: the ~64 workgroups resident on an XCD at any time are
    // consecutive owner blocks of the SAME split, i.e. they stream the same "other" tiles in the same order and share them in that
    // XCD's L2 (owner-block-major order put every split on every XCD: 7.1 GB of L2 misses per launch at configs[1]).
    // plan_multi pads every group to a multiple of 8 workgroups (blk0 % 8 == 0); the padding workgroups exit here.
    const int wg_in_grp = (int)blockIdx.x - grp.blk0;
    const int nsplit = grp.nsplit, n_ob = (grp.nown + S16_OWN - 1) / S16_OWN, n_units = n_ob * nsplit;
    const int unit = (wg_in_grp & 7) * ((n_units + 7) >> 3) + (wg_in_grp >> 3);
    if ((wg_in_grp >> 3) >= ((n_units + 7) >> 3) || unit >= n_units) return;
    const int split = unit / n_ob;
    const int own0 = grp.own0 + (unit - split * n_ob) * S16_OWN;
    const int own_end = grp.own0 + grp.nown;
    const int my_i = own0 + wave * 16 + l15;
    const bool iv = my_i < own_end;

    f32x4 own[M][6];
    float ownt[M][NTL], beta[M];
#pragma unroll
    for (int m = 0; m < M; ++m) {
        const float* src = a.Z[m] + (size_t)(iv ? my_i : own0) * DP;
        const float msk = iv ? a.k1 : 0.f;                      // pre-scaled: S arrives as the tau1 exp2 argument
#pragma unroll
        for (int q = 0; q < 6; ++q) own[m][q] = *reinterpret_cast<const f32x4*>(src + 16 * q + 4 * g4) * msk;   // k = 16q + 4g4 + r
#pragma unroll
        for (int t = 0; t < NTL; ++t) ownt[m][t] = src[96 + 4 * t + ((t == 1 && a.swap_tail) ? (g4 ^ 1) : g4)] * msk;      // k = 96 + 4t + g4
        beta[m] = a.beta[m];
    }
    f32x4 gacc[GRAD ? M : 1][NCT];
#pragma unroll
    for (int m = 0; m < (GRAD ? M : 1); ++m)
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct) gacc[m][ct] = f32x4{0.f, 0.f, 0.f, 0.f};
    float gam[M];
#pragma unroll
    for (int m = 0; m < M; ++m) gam[m] = 0.f;
    // exp2 arguments from an S value `sv` as the MFMA delivers it (already times log2(e)/tau1):  tau1 term exp2(sv),  tau0 term exp2(sv * ka)
    const float ka = to_sgpr(a.k0 / a.k1);
    auto e0 = [&](float sv) { return fexp2(sv * ka); };
    auto e1 = [&](float sv) { return fexp2(sv); };

    const int wave_u = __builtin_amdgcn_readfirstlane(wave);        // M0 (the DMA's LDS address) must be provably uniform
    // A tile is M x 13 chunks of 1 KiB (64 lanes x 16 B).  Wave w fetches chunks (w + m) % WAVES + WAVES * k of table m: the table index is
    // a compile-time constant of every DMA (its base pointer stays in two SGPRs) and the chunk offset is one uniform value plus a
    // literal.  (Chunk c = c0 + wave over the flattened M x 13 list made the table a run-time index: an s_load of a.Z[m] from the
    // kernel arguments + s_waitcnt before each of the 10 DMAs of every tile, and 80 loop-invariant SGPRs, half of them spilled.)
    auto issue = [&](int j0, float* buf) {
        int l4 = threadIdx.x;
        asm volatile("" : "+v"(l4));      // lane offset recomputed here (2 VALU): as a loop invariant it is folded into per-lane 64-bit bases that
        l4 = (l4 & 63) * 4;               // get spilled, and a scratch reload's vmcnt(0) in front of the DMAs serialises them
#pragma unroll
        for (int m = 0; m < M; ++m) {
            const int rot = (wave_u + m) & (S16_WAVES - 1);
            const float* src = a.Z[m] + ((size_t)j0 * DP + rot * 256) + l4;    // uniform base (SGPR pair) + lane offset
            float* dst = buf + m * TILE_F + rot * 256;
#pragma unroll
            for (int k = 0; k * S16_WAVES < 13; ++k) {
                if ((k + 1) * S16_WAVES > 13 && rot + k * S16_WAVES >= 13) break;      // uniform; only the last k can fall off the table
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src + k * S16_WAVES * 256),
                                                 (__attribute__((address_space(3))) void*)(dst + k * S16_WAVES * 256), 16, 0, 0);
            }
        }
    };
    // this lane's other rows inside a 32-row tile: element (jh, r) <-> row jh*16 + pi(4*g4 + r)
    int jrow[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) jrow[r] = s16_pi(4 * g4 + r);
    const int arow = s16_pi(l15);                                  // the other row this lane feeds as MFMA A operand

#pragma unroll
    for (int sg = 0; sg < 2; ++sg) {
        if (sg >= grp.nseg) break;
        const SweepSeg seg = grp.seg[sg];
        const int ntile = (seg.n + OT - 1) / OT;
        const int j_end = seg.row0 + seg.n;
        float c0[M + 1], c1[M + 1];
#pragma unroll
        for (int m = 0; m <= M; ++m) {                      // uniform, but fp64 arithmetic leaves them in VGPRs: 2 (M + 1) registers of a full file
            c0[m] = GRAD ? to_sgpr((float)(a.gs[m * 8 + seg.fam * 2 + 0] * (double)a.it0)) : 0.f;
            c1[m] = GRAD ? to_sgpr((float)(a.gs[m * 8 + seg.fam * 2 + 1] * (double)a.it1)) : 0.f;
        }
        double dsum[M + 1][2];
#pragma unroll
        for (int m = 0; m <= M; ++m) { dsum[m][0] = 0.0; dsum[m][1] = 0.0; }

        __syncthreads();
        if (split < ntile) issue(seg.row0 + split * OT, lds);
        int it = 0;
        for (int jt = split; jt < ntile; jt += nsplit, ++it) {
            float* buf = lds + (it & 1) * BUF_F;
            const int j0 = seg.row0 + jt * OT;
            __syncthreads();                               // tile `it` landed / other buffer free
            if (jt + nsplit < ntile) issue(seg.row0 + (jt + nsplit) * OT, lds + ((it + 1) & 1) * BUF_F);
            if (GRAD && j0 + OT > j_end) {
                // Last, partial tile of a segment (uniform, once per segment): the rows past the segment's end hold the next segment's
                // data.  Zeroing them in LDS makes every one of their contributions vanish by itself -- S = 0, c * 0 added to the owner
                // gradient, 0 added to Gamma -- so the gradient epilogue needs no per-element validity mask at all.
                const int nval = j_end - j0;
                for (int x = tid; x < M * (OT - nval) * (DP / 4); x += S16_THREADS) {
                    const int m = x / ((OT - nval) * (DP / 4)), rem = x - m * ((OT - nval) * (DP / 4));
                    *reinterpret_cast<f32x4*>(buf + m * TILE_F + nval * DP + rem * 4) = f32x4{0.f, 0.f, 0.f, 0.f};
                }
                __syncthreads();
            }

            // ---- S^T tiles of the M tables: lane&15 = owner row, (g4, r) = other row.
            // Per 16-row half the M accumulation chains are interleaved (a dependent MFMA is M issues away) and the
            // A operands are read one K group ahead into the other of two register sets (assigning alternately, never
            // copying, keeps hipcc from folding the two sets back into one load->wait->use chain).
            f32x4 sacc[M][2];
#pragma unroll
            for (int jh = 0; jh < 2; ++jh) {
                const float* ap = buf + (jh * 16 + arow) * DP + 4 * g4;
                const float* at = buf + (jh * 16 + arow) * DP + 96 + g4;
                f32x4 avA[M], avB[M];
                float tl[M][NTL];
#pragma unroll
                for (int m = 0; m < M; ++m) {
                    sacc[m][jh] = f32x4{0.f, 0.f, 0.f, 0.f};
                    avA[m] = *reinterpret_cast<const f32x4*>(ap + m * TILE_F);
                    avB[m] = avA[m];
                }
                __builtin_amdgcn_sched_group_barrier(0x100, M, 0);
#pragma unroll
                for (int q = 0; q < 6; ++q) {
                    if (q < 5) {
#pragma unroll
                        for (int m = 0; m < M; ++m) {
                            if (q & 1) avA[m] = *reinterpret_cast<const f32x4*>(ap + m * TILE_F + 16 * (q + 1));
                            else avB[m] = *reinterpret_cast<const f32x4*>(ap + m * TILE_F + 16 * (q + 1));
                        }
                    } else {
#pragma unroll
                        for (int m = 0; m < M; ++m)
#pragma unroll
                            for (int t = 0; t < NTL; ++t) tl[m][t] = at[m * TILE_F + 4 * t];
                    }
#pragma unroll
                    for (int r = 0; r < 4; ++r)
#pragma unroll
                        for (int m = 0; m < M; ++m)
                            sacc[m][jh] = __builtin_amdgcn_mfma_f32_16x16x4f32((q & 1) ? avB[m][r] : avA[m][r], own[m][q][r], sacc[m][jh], 0, 0, 0);
                    if (q < 5) __builtin_amdgcn_sched_group_barrier(0x100, M, 0);          // next group's reads first ...
                    else __builtin_amdgcn_sched_group_barrier(0x100, NTL * M, 0);
                    __builtin_amdgcn_sched_group_barrier(0x008, 4 * M, 0);                 // ... then this group's MFMAs
                }
#pragma unroll
                for (int t = 0; t < NTL; ++t) {
                    if (t >= a.ktail) break;                       // uniform: an all-zero padding step is skipped (exact)
#pragma unroll
                    for (int m = 0; m < M; ++m)
                        sacc[m][jh] = __builtin_amdgcn_mfma_f32_16x16x4f32(tl[m][t], ownt[m][t], sacc[m][jh], 0, 0, 0);
                }
            }

            if (!GRAD) {
                float p0[M + 1], p1[M + 1];
#pragma unroll
                for (int m = 0; m <= M; ++m) { p0[m] = 0.f; p1[m] = 0.f; }
                // interior tiles (every owner row of the block and every other row of the tile valid) add unmasked
                auto sums_tile = [&](auto masked_c) {
                    constexpr bool MASKED = decltype(masked_c)::value;
#pragma unroll
                    for (int jh = 0; jh < 2; ++jh)
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const float okf = (!MASKED || (iv && (j0 + jh * 16 + jrow[r] < j_end))) ? 1.f : 0.f;
                            float sj = 0.f;
#pragma unroll
                            for (int m = 0; m < M; ++m) {
                                const float sv = sacc[m][jh][r];
                                sj = fmaf(beta[m], sv, sj);
                                p0[m] = MASKED ? fmaf(okf, e0(sv), p0[m]) : p0[m] + e0(sv);
                                p1[m] = MASKED ? fmaf(okf, e1(sv), p1[m]) : p1[m] + e1(sv);
                            }
                            p0[M] = MASKED ? fmaf(okf, e0(sj), p0[M]) : p0[M] + e0(sj);
                            p1[M] = MASKED ? fmaf(okf, e1(sj), p1[M]) : p1[M] + e1(sj);
                        }
                };
                if (j0 + OT <= j_end && own0 + S16_OWN <= own_end) sums_tile(std::false_type{}); else sums_tile(std::true_type{});   // uniform
#pragma unroll
                for (int m = 0; m <= M; ++m) { dsum[m][0] += (double)p0[m]; dsum[m][1] += (double)p1[m]; }
            } else {
                // No validity masks here: rows past a segment's end were zeroed in LDS above, and owner rows past the group's end carry
                // zero operands and are never written back.
                float cj[2][4];
#pragma unroll
                for (int jh = 0; jh < 2; ++jh)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        float sj = 0.f;
#pragma unroll
                        for (int m = 0; m < M; ++m) sj = fmaf(beta[m], sacc[m][jh][r], sj);
                        cj[jh][r] = c0[M] * e0(sj) + c1[M] * e1(sj);
                    }
                if (g < 2) {                                    // Gamma_m = sum dL/dS_J * S_m, each pair once (anchor-owner sweep)
#pragma unroll
                    for (int m = 0; m < M; ++m)
#pragma unroll
                        for (int jh = 0; jh < 2; ++jh)
#pragma unroll
                            for (int r = 0; r < 4; ++r) gam[m] = fmaf(cj[jh][r], sacc[m][jh][r], gam[m]);
                }
                // c_m = dL/dS_m + beta_m dL/dS_J, then dZ_m[own, :] += c_m * Z_m[other, :].  The M*8 (table, other row)
                // steps are software pipelined: while step e's 7 MFMAs issue, step e+1's coefficient (2 exp2 + ~8 VALU)
                // and its 7 B operands (ds_read_b32) are produced into the other register set.
                float cmv[2], bv[2][NCT];
                auto coef = [&](int e) {
                    const int m = e >> 3, jh = (e >> 2) & 1, r = e & 3;
                    const float sv = sacc[m][jh][r];
                    return fmaf(beta[m], cj[jh][r], c0[m] * e0(sv) + c1[m] * e1(sv));
                };
                auto bload = [&](int e, float* dst) {
                    const int m = e >> 3, jh = (e >> 2) & 1, r = e & 3;
                    const float* bb = buf + m * TILE_F + (jh * 16 + jrow[r]) * DP + l15;
#pragma unroll
                    for (int ct = 0; ct < NCT; ++ct) dst[ct] = bb[ct * 16];
                };
                cmv[0] = coef(0);
                bload(0, bv[0]);
#pragma unroll
                for (int e = 0; e < M * 8; ++e) {
                    if (e + 1 < M * 8) { cmv[(e + 1) & 1] = coef(e + 1); bload(e + 1, bv[(e + 1) & 1]); }
#pragma unroll
                    for (int ct = 0; ct < NCT; ++ct)
                        gacc[GRAD ? (e >> 3) : 0][ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(cmv[e & 1], bv[e & 1][ct], gacc[GRAD ? (e >> 3) : 0][ct], 0, 0, 0);
#pragma unroll
                    for (int ct = 0; ct < NCT; ++ct) {
                        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                        __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
                        __builtin_amdgcn_sched_group_barrier(0x002, 2, 0);
                    }
                }
#pragma unroll
                for (int m = 0; m < M; ++m) asm volatile("" : "+v"(gam[m]));     // keep the updates out of the loop latch
            }
        }
        if (!GRAD) {
#pragma unroll
            for (int m = 0; m <= M; ++m)
#pragma unroll
                for (int tt = 0; tt < 2; ++tt) {
                    const double v = wave_sum_d(dsum[m][tt]);
                    if (lane == 0 && v != 0.0) atomicAdd(a.sums + (M + 1) * 8 * (1 + my_slot()) + m * 8 + seg.fam * 2 + tt, v);
                }
        }
    }
    if (GRAD) {
#pragma unroll
        for (int m = 0; m < M; ++m) {
            float* dz = a.dZ[m];
#pragma unroll
            for (int ct = 0; ct < NCT; ++ct) {
                const int d = ct * 16 + l15;
                if (d < DP) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int i = own0 + wave * 16 + 4 * g4 + r;
                        if (i < own_end) atomicAdd(dz + (size_t)i * DP + d, gacc[GRAD ? m : 0][ct][r]);
                    }
                }
            }
        }
        if (g < 2) {
#pragma unroll
            for (int m = 0; m < M; ++m) {
                const float v = wave_sum(gam[m]) / a.k1;       // Gamma was accumulated on pre-scaled S values
                if (lane == 0 && v != 0.f) atomicAdd(a.gamma + M * (1 + my_slot()) + m, (double)v);
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------
// M = 4 (point + gat + rel + attr: the module list of every config the reference ships) on PAIRED waves.
//
// sweep16_kernel<4> needs 104 owner-operand + 112 gradient-accumulator + 32 S-tile registers per lane: one wave per SIMD, so
// nothing runs under a wave's epilogue or barrier wait (0.61 of the MFMA peak against 0.72 for M = 3 with two waves per SIMD).
// Here a workgroup still owns 64 rows but runs 8 waves: wave (rg, th) owns row group rg (16 rows) and TABLES {2 th, 2 th + 1} only --
// half of the operands, S tiles and accumulators (~200 registers: two waves per SIMD again).  The joint similarity needs all four
// S tiles of an element, so the two waves of a row group swap their halves through LDS once per tile (16 values per lane each way,
// one extra workgroup barrier -- a pairwise LDS-flag hand-over instead measured 2 % slower: the spinning wave takes issue slots);
// the joint coefficient is then computed by both (the only duplicated work, ~100 VALU per tile) and
// each wave forms the coefficients and gradient GEMMs of its own two tables.  Same work units, XCD order and DMA ring as sweep16_kernel.
// ------------------------------------------------------------------------------------------------
constexpr int S4_THREADS = 512;
template <bool GRAD>
__global__ __launch_bounds__(S4_THREADS, 1) void sweep16x2_kernel(MultiArgs a) {
    constexpr int M = 4, MT = 2, DP = 104, OT = 32, NCT = 7;
    constexpr int TILE_F = OT * DP, BUF_F = M * TILE_F;
    extern __shared__ __attribute__((aligned(16))) float lds[];     // [2][M][OT][DP] + 32 slack + exchange [8 waves][16][64]
    float* xbuf = lds + 2 * BUF_F + 32;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g4 = lane >> 4, l15 = lane & 15;
    const int rg = wave & 3, th = wave >> 2;                        // row group, table half
    int g = 0;
#pragma unroll
    for (int i = 1; i < 4; ++i) if (i < a.ngroups && (int)blockIdx.x >= a.grp[i].blk0) g = i;
    const SweepGroup& grp = a.grp[g];
    const int wg_in_grp = (int)blockIdx.x - grp.blk0;
    const int nsplit = grp.nsplit, n_ob = (grp.nown + S16_OWN - 1) / S16_OWN, n_units = n_ob * nsplit;
    const int unit = (wg_in_grp & 7) * ((n_units + 7) >> 3) + (wg_in_grp >> 3);     // XCD-aware order, see sweep16_kernel
    if ((wg_in_grp >> 3) >= ((n_units + 7) >> 3) || unit >= n_units) return;
    const int split = unit / n_ob;
    const int own0 = grp.own0 + (unit - split * n_ob) * S16_OWN;
    const int own_end = grp.own0 + grp.nown;
    const int my_i = own0 + rg * 16 + l15;
    const bool iv = my_i < own_end;

    f32x4 own[MT][6];
    float ownt[MT][2], bm[MT], bp[MT];                             // beta of this wave's tables / of its partner's
#pragma unroll
    for (int m = 0; m < MT; ++m) {
        const float* src = a.Z[2 * th + m] + (size_t)(iv ? my_i : own0) * DP;
        const float msk = iv ? a.k1 : 0.f;                      // pre-scaled owner rows, as in sweep16_kernel
#pragma unroll
        for (int q = 0; q < 6; ++q) own[m][q] = *reinterpret_cast<const f32x4*>(src + 16 * q + 4 * g4) * msk;
#pragma unroll
        for (int t = 0; t < 2; ++t) ownt[m][t] = src[96 + 4 * t + ((t == 1 && a.swap_tail) ? (g4 ^ 1) : g4)] * msk;
    }
#pragma unroll
    for (int m = 0; m < MT; ++m) { bm[m] = a.beta[2 * th + m]; bp[m] = a.beta[2 * (1 - th) + m]; }
    f32x4 gacc[GRAD ? MT : 1][NCT];
#pragma unroll
    for (int m = 0; m < (GRAD ? MT : 1); ++m)
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct) gacc[m][ct] = f32x4{0.f, 0.f, 0.f, 0.f};
    float gam[MT] = {0.f, 0.f};
    const float ka = a.k0 / a.k1;                                  // S arrives times log2(e)/tau1: tau1 term exp2(sv), tau0 term exp2(sv * ka)
    auto e0 = [&](float sv) { return fexp2(sv * ka); };
    auto e1 = [&](float sv) { return fexp2(sv); };

    const int wave_u = __builtin_amdgcn_readfirstlane(wave);
    auto issue = [&](int j0, float* buf) {      // chunk (wave + 2m) % 8 (+ 8) of table m: compile-time table index, see sweep16_kernel
        int l4 = threadIdx.x;
        asm volatile("" : "+v"(l4));
        l4 = (l4 & 63) * 4;
#pragma unroll
        for (int m = 0; m < M; ++m) {
            const int rot = (wave_u + 2 * m) & 7;
            const float* src = a.Z[m] + ((size_t)j0 * DP + rot * 256) + l4;
            float* dst = buf + m * TILE_F + rot * 256;
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                if (k == 1 && rot + 8 >= 13) break;            // uniform
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src + k * 8 * 256),
                                                 (__attribute__((address_space(3))) void*)(dst + k * 8 * 256), 16, 0, 0);
            }
        }
    };
    int jrow[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) jrow[r] = s16_pi(4 * g4 + r);
    const int arow = s16_pi(l15);
    float* xmine = xbuf + ((rg * 2 + th) * 16) * 64 + lane;
    const float* xpart = xbuf + ((rg * 2 + (1 - th)) * 16) * 64 + lane;

#pragma unroll
    for (int sg = 0; sg < 2; ++sg) {
        if (sg >= grp.nseg) break;
        const SweepSeg seg = grp.seg[sg];
        const int ntile = (seg.n + OT - 1) / OT;
        const int j_end = seg.row0 + seg.n;
        float c0[MT + 1], c1[MT + 1];                              // this wave's two tables, then the joint table
#pragma unroll
        for (int m = 0; m <= MT; ++m) {
            const int tab = m == MT ? M : 2 * th + m;
            c0[m] = GRAD ? (float)(a.gs[tab * 8 + seg.fam * 2 + 0] * (double)a.it0) : 0.f;
            c1[m] = GRAD ? (float)(a.gs[tab * 8 + seg.fam * 2 + 1] * (double)a.it1) : 0.f;
        }
        double dsum[MT + 1][2];                                    // own two tables + this wave's half of the joint table
#pragma unroll
        for (int m = 0; m <= MT; ++m) { dsum[m][0] = 0.0; dsum[m][1] = 0.0; }

        __syncthreads();
        if (split < ntile) issue(seg.row0 + split * OT, lds);
        int it = 0;
        for (int jt = split; jt < ntile; jt += nsplit, ++it) {
            float* buf = lds + (it & 1) * BUF_F;
            const int j0 = seg.row0 + jt * OT;
            __syncthreads();                               // tile `it` landed / other buffer free / exchange buffer free
            if (jt + nsplit < ntile) issue(seg.row0 + (jt + nsplit) * OT, lds + ((it + 1) & 1) * BUF_F);
            if (GRAD && j0 + OT > j_end) {                 // partial last tile of a segment: zero the rows past its end (see sweep16_kernel)
                const int nval = j_end - j0;
                for (int x = tid; x < M * (OT - nval) * (DP / 4); x += S4_THREADS) {
                    const int m = x / ((OT - nval) * (DP / 4)), rem = x - m * ((OT - nval) * (DP / 4));
                    *reinterpret_cast<f32x4*>(buf + m * TILE_F + nval * DP + rem * 4) = f32x4{0.f, 0.f, 0.f, 0.f};
                }
                __syncthreads();
            }

            // ---- S^T tiles of this wave's two tables
            f32x4 mine[MT][2], part[MT][2];
#pragma unroll
            for (int jh = 0; jh < 2; ++jh) {
                const float* ap = buf + (2 * th) * TILE_F + (jh * 16 + arow) * DP + 4 * g4;
                const float* at = buf + (2 * th) * TILE_F + (jh * 16 + arow) * DP + 96 + g4;
                f32x4 sacc[MT], avA[MT], avB[MT];
                float tl[MT][2];
#pragma unroll
                for (int m = 0; m < MT; ++m) {
                    sacc[m] = f32x4{0.f, 0.f, 0.f, 0.f};
                    avA[m] = *reinterpret_cast<const f32x4*>(ap + m * TILE_F);
                    avB[m] = avA[m];
                }
                __builtin_amdgcn_sched_group_barrier(0x100, MT, 0);
#pragma unroll
                for (int q = 0; q < 6; ++q) {
                    if (q < 5) {
#pragma unroll
                        for (int m = 0; m < MT; ++m) {
                            if (q & 1) avA[m] = *reinterpret_cast<const f32x4*>(ap + m * TILE_F + 16 * (q + 1));
                            else avB[m] = *reinterpret_cast<const f32x4*>(ap + m * TILE_F + 16 * (q + 1));
                        }
                    } else {
#pragma unroll
                        for (int m = 0; m < MT; ++m) { tl[m][0] = at[m * TILE_F]; tl[m][1] = at[m * TILE_F + 4]; }
                    }
#pragma unroll
                    for (int r = 0; r < 4; ++r)
#pragma unroll
                        for (int m = 0; m < MT; ++m)
                            sacc[m] = __builtin_amdgcn_mfma_f32_16x16x4f32((q & 1) ? avB[m][r] : avA[m][r], own[m][q][r], sacc[m], 0, 0, 0);
                    if (q < 5) __builtin_amdgcn_sched_group_barrier(0x100, MT, 0);
                    else __builtin_amdgcn_sched_group_barrier(0x100, 2 * MT, 0);
                    __builtin_amdgcn_sched_group_barrier(0x008, 4 * MT, 0);
                }
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    if (t >= a.ktail) break;
#pragma unroll
                    for (int m = 0; m < MT; ++m)
                        sacc[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(tl[m][t], ownt[m][t], sacc[m], 0, 0, 0);
                }
#pragma unroll
                for (int m = 0; m < MT; ++m) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) xmine[((m * 2 + jh) * 4 + r) * 64] = sacc[m][r];
                    mine[m][jh] = sacc[m];
                }
            }
            __syncthreads();                               // both halves of every row group are in the exchange buffer
#pragma unroll
            for (int m = 0; m < MT; ++m)
#pragma unroll
                for (int jh = 0; jh < 2; ++jh) {
                    f32x4 v;
#pragma unroll
                    for (int r = 0; r < 4; ++r) v[r] = xpart[((m * 2 + jh) * 4 + r) * 64];
                    part[m][jh] = v;
                }

            if (!GRAD) {
                float p0[MT + 1], p1[MT + 1];
#pragma unroll
                for (int m = 0; m <= MT; ++m) { p0[m] = 0.f; p1[m] = 0.f; }
#pragma unroll
                for (int jh = 0; jh < 2; ++jh)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float okf = (iv && (j0 + jh * 16 + jrow[r] < j_end)) ? 1.f : 0.f;
                        float sj = 0.f;
#pragma unroll
                        for (int m = 0; m < MT; ++m) sj = fmaf(bm[m], mine[m][jh][r], fmaf(bp[m], part[m][jh][r], sj));
#pragma unroll
                        for (int m = 0; m < MT; ++m) {
                            const float sv = mine[m][jh][r];
                            p0[m] = fmaf(okf, e0(sv), p0[m]);
                            p1[m] = fmaf(okf, e1(sv), p1[m]);
                        }
                        if (jh == th) {                             // wave-uniform: the joint table's sums, one 16-row half per partner
                            p0[MT] = fmaf(okf, e0(sj), p0[MT]);
                            p1[MT] = fmaf(okf, e1(sj), p1[MT]);
                        }
                    }
#pragma unroll
                for (int m = 0; m <= MT; ++m) { dsum[m][0] += (double)p0[m]; dsum[m][1] += (double)p1[m]; }
            } else {
                float cj[2][4];                             // no validity masks: see sweep16_kernel
#pragma unroll
                for (int jh = 0; jh < 2; ++jh)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        float sj = 0.f;
#pragma unroll
                        for (int m = 0; m < MT; ++m) sj = fmaf(bm[m], mine[m][jh][r], fmaf(bp[m], part[m][jh][r], sj));
                        cj[jh][r] = c0[MT] * e0(sj) + c1[MT] * e1(sj);
                    }
                if (g < 2) {
#pragma unroll
                    for (int m = 0; m < MT; ++m)
#pragma unroll
                        for (int jh = 0; jh < 2; ++jh)
#pragma unroll
                            for (int r = 0; r < 4; ++r) gam[m] = fmaf(cj[jh][r], mine[m][jh][r], gam[m]);
                }
                float cmv[2], bv[2][NCT];
                auto coef = [&](int e) {
                    const int m = e >> 3, jh = (e >> 2) & 1, r = e & 3;
                    const float sv = mine[m][jh][r];
                    return fmaf(bm[m], cj[jh][r], c0[m] * e0(sv) + c1[m] * e1(sv));
                };
                auto bload = [&](int e, float* dst) {
                    const int m = e >> 3, jh = (e >> 2) & 1, r = e & 3;
                    const float* bb = buf + (2 * th + m) * TILE_F + (jh * 16 + jrow[r]) * DP + l15;
#pragma unroll
                    for (int ct = 0; ct < NCT; ++ct) dst[ct] = bb[ct * 16];
                };
                cmv[0] = coef(0);
                bload(0, bv[0]);
#pragma unroll
                for (int e = 0; e < MT * 8; ++e) {
                    if (e + 1 < MT * 8) { cmv[(e + 1) & 1] = coef(e + 1); bload(e + 1, bv[(e + 1) & 1]); }
#pragma unroll
                    for (int ct = 0; ct < NCT; ++ct)
                        gacc[GRAD ? (e >> 3) : 0][ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(cmv[e & 1], bv[e & 1][ct], gacc[GRAD ? (e >> 3) : 0][ct], 0, 0, 0);
#pragma unroll
                    for (int ct = 0; ct < NCT; ++ct) {
                        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                        __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
                        __builtin_amdgcn_sched_group_barrier(0x002, 2, 0);
                    }
                }
#pragma unroll
                for (int m = 0; m < MT; ++m) asm volatile("" : "+v"(gam[m]));
            }
        }
        if (!GRAD) {
#pragma unroll
            for (int m = 0; m <= MT; ++m) {
                const int tab = m == MT ? M : 2 * th + m;
#pragma unroll
                for (int tt = 0; tt < 2; ++tt) {
                    const double v = wave_sum_d(dsum[m][tt]);
                    if (lane == 0 && v != 0.0) atomicAdd(a.sums + (M + 1) * 8 * (1 + my_slot()) + tab * 8 + seg.fam * 2 + tt, v);
                }
            }
        }
    }
    if (GRAD) {
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            float* dz = a.dZ[2 * th + m];
#pragma unroll
            for (int ct = 0; ct < NCT; ++ct) {
                const int d = ct * 16 + l15;
                if (d < DP) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int i = own0 + rg * 16 + 4 * g4 + r;
                        if (i < own_end) atomicAdd(dz + (size_t)i * DP + d, gacc[GRAD ? m : 0][ct][r]);
                    }
                }
            }
        }
        if (g < 2) {
#pragma unroll
            for (int m = 0; m < MT; ++m) {
                const float v = wave_sum(gam[m]) / a.k1;       // accumulated on pre-scaled S values
                if (lane == 0 && v != 0.f) atomicAdd(a.gamma + M * (1 + my_slot()) + 2 * th + m, (double)v);
            }
        }
    }
}

template <bool GRAD>
static void launch_sweep16x2(const MultiArgs& a, int nwg, hipStream_t s) {
    const size_t lds = ((size_t)2 * 4 * 32 * 104 + 32 + 8 * 16 * 64) * sizeof(float);
    auto k = sweep16x2_kernel<GRAD>;
    hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(k, dim3(nwg), dim3(S4_THREADS), lds, s, a);
}

template <int M, bool GRAD>
static void launch_sweep16(const MultiArgs& a, int nwg, hipStream_t s) {
    const size_t lds = ((size_t)2 * M * 32 * 104 + 32) * sizeof(float);
    auto k = a.ktail > 1 ? sweep16_kernel<M, GRAD, true> : sweep16_kernel<M, GRAD, false>;
    hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(k, dim3(nwg), dim3(S16_THREADS), lds, s, a);
}

// poison = NaN if any row of any table took F.normalize's eps branch (then S_J != sum beta_m S_m)
__global__ void check_norms_kernel(const float* __restrict__ nrm, int n, float* __restrict__ poison) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
        if (!(nrm[i] >= 1e-12f)) *poison = __builtin_nanf("");
}

int rows_grid(int R) {
    int g = (R + 3) / 4;
    const int cap = sga_num_cus() * 8;
    return g > cap ? cap : (g < 1 ? 1 : g);
}

}  // namespace

extern "C" int sga_loss_gather(const float* E, int T, int D, const int32_t* idx, int R, float* Z, int Dp, float* nrm,
                               void* stream) {
    (void)T;
    SGA_CHECK_ARG(D >= 1 && Dp >= D && Dp % 8 == 0 && R >= 0, "sga_loss_gather: bad argument (Dp must be a multiple of 8 >= D)");
    if (R == 0) return SGA_OK;
    SGA_CHECK_ARG(E && idx && Z && nrm, "sga_loss_gather: null pointer");
    hipLaunchKernelGGL(gather_normalize_kernel, dim3(rows_grid(R)), dim3(256), 0, static_cast<hipStream_t>(stream), E, D, idx, R, Z, Dp, nrm);
    SGA_CHECK_LAUNCH("sga_loss_gather");
    return SGA_OK;
}

extern "C" int sga_loss_scatter(const float* dZ, const float* Z, const float* nrm, const int32_t* idx, int R, int D,
                                int Dp, float* dE, void* stream) {
    SGA_CHECK_ARG(D >= 1 && Dp >= D && R >= 0, "sga_loss_scatter: bad argument");
    if (R == 0) return SGA_OK;
    SGA_CHECK_ARG(dZ && Z && nrm && idx && dE, "sga_loss_scatter: null pointer");
    hipLaunchKernelGGL(scatter_normalize_bwd_kernel, dim3(rows_grid(R)), dim3(256), 0, static_cast<hipStream_t>(stream), dZ, Z, nrm, idx, R, D, Dp, dE);
    SGA_CHECK_LAUNCH("sga_loss_scatter");
    return SGA_OK;
}

// ---- fused multi-table entry points (joint table == fusion of the M tables) ----------------------------
static int fill_multi(MultiArgs& a, const float* const* Z, int M, int D, const float* beta, int A, int J1, int J2, float tau0,
                      float tau1, bool grad, int a_lo, int a_hi) {
    if (D < 1 || D > 104) { sga_set_error("sga_loss_multi: D=%d outside [1,104] (the fused sweeps take Dp = 104 tables)", D); return SGA_ERR_ARG; }
    a.ktail = D > 100 ? 2 : (D > 96 ? 1 : 0);
    if (a_lo < 0 || a_hi > A || a_lo > a_hi) { sga_set_error("sga_loss_multi: anchor shard [%d,%d) outside [0,%d]", a_lo, a_hi, A); return SGA_ERR_ARG; }
    if (M < 2 || M > 4) { sga_set_error("sga_loss_multi: M=%d outside [2,4]", M); return SGA_ERR_ARG; }
    a.M = M;
    for (int m = 0; m < M; ++m) { if (!Z[m]) { sga_set_error("sga_loss_multi: null table"); return SGA_ERR_ARG; } a.Z[m] = Z[m]; }
    a.beta = beta; a.k0 = LOG2E / tau0; a.k1 = LOG2E / tau1; a.it0 = 1.f / tau0; a.it1 = 1.f / tau1;
    a.ngroups = fill_groups(a.grp, A, J1, J2, grad, a_lo, a_hi);
    return SGA_OK;
}
// Split every group's other-tile list so that all workgroups run ~`target` 32-row steps: uniform work units keep
// the 256 CUs busy to the end (anchor-owner blocks see 2.4x more other rows than negative-owner blocks).
static int plan_multi(MultiArgs& a, int target_steps, int own_rows = 128) {
    int nwg = 0;
    for (int g = 0; g < a.ngroups; ++g) {
        SweepGroup& G = a.grp[g];
        int steps = 0;
        for (int sg = 0; sg < G.nseg; ++sg) steps += (G.seg[sg].n + 31) / 32;
        int ns = (steps + target_steps - 1) / target_steps;
        if (ns < 1) ns = 1;
        G.nsplit = ns;
        G.blk0 = nwg;
        nwg += ((((G.nown + own_rows - 1) / own_rows) * ns + 7) / 8) * 8;      // 8 per-XCD chunks (sweep16_kernel's work order)
    }
    return nwg;
}

static int multi_sums_impl(const float* const* Z, int M, int D, bool centred, const float* beta, int A, int J1, int J2, float tau0,
                           float tau1, double* sums, int a_lo, int a_hi, void* stream) {
    SGA_CHECK_ARG(Z && beta && sums && A >= 0 && J1 >= 0 && J2 >= 0, "sga_loss_multi_sums: bad argument");
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (int rc0 = zero_slots(sums, (M + 1) * 8, s, "sga_loss_multi_sums")) return rc0;
    if (A == 0 || a_hi <= a_lo || (J1 == 0 && J2 == 0)) return SGA_OK;
    MultiArgs a{};
    int rc = fill_multi(a, Z, M, D, beta, A, J1, J2, tau0, tau1, false, a_lo, a_hi);
    if (rc) return rc;
    a.swap_tail = centred ? 1 : 0;
    a.sums = sums;
    const int nwg = plan_multi(a, 160, S16_OWN);
    if (M == 2) launch_sweep16<2, false>(a, nwg, s);
    else if (M == 3) launch_sweep16<3, false>(a, nwg, s);
    else launch_sweep16x2<false>(a, nwg, s);
    fold_slots(sums, (M + 1) * 8, s);
    SGA_CHECK_LAUNCH("sga_loss_multi_sums");
    return SGA_OK;
}
extern "C" int sga_loss_multi_sums(const float* const* Z, int M, int D, const float* beta, int A, int J1, int J2, float tau0,
                                   float tau1, double* sums, int a_lo, int a_hi, void* stream) {
    return multi_sums_impl(Z, M, D, false, beta, A, J1, J2, tau0, tau1, sums, a_lo, a_hi, stream);
}
// The same sweeps over CENTRED tables Zc (sga_loss_centre_tables: 100 data columns of z - zbar, column 100 = b, 101 = 1): identical
// similarities (the owner's swapped K tail adds b_i + b_j), gradient delivered in two parts -- dZ[:, 0..99] = sum c (z - zbar),
// dZ[:, 101] = sum c -- for sga_loss_scatter_tangent_stat.
extern "C" int sga_loss_multi_sums_centred(const float* const* Zc, int M, const float* beta, int A, int J1, int J2, float tau0,
                                           float tau1, double* sums, int a_lo, int a_hi, void* stream) {
    return multi_sums_impl(Zc, M, 102, true, beta, A, J1, J2, tau0, tau1, sums, a_lo, a_hi, stream);
}

static int multi_grad_impl(const float* const* Z, int M, int D, bool centred, const float* beta, int A, int J1, int J2, float tau0,
                           float tau1, const double* gs, float* const* dZ, double* gamma, int a_lo, int a_hi,
                           void* stream) {
    SGA_CHECK_ARG(Z && beta && gs && dZ && gamma && A >= 0 && J1 >= 0 && J2 >= 0, "sga_loss_multi_grad: bad argument");
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (int rcz = zero_slots(gamma, M > 0 ? M : 1, s, "sga_loss_multi_grad")) return rcz;
    if (A == 0 || a_hi <= a_lo || (J1 == 0 && J2 == 0)) return SGA_OK;
    MultiArgs a{};
    int rc = fill_multi(a, Z, M, D, beta, A, J1, J2, tau0, tau1, true, a_lo, a_hi);
    if (rc) return rc;
    a.swap_tail = centred ? 1 : 0;
    a.gs = gs; a.gamma = gamma;
    for (int m = 0; m < M; ++m) { SGA_CHECK_ARG(dZ[m], "sga_loss_multi_grad: null dZ"); a.dZ[m] = dZ[m]; }
    const int nwg = plan_multi(a, 160, S16_OWN);
    if (M == 2) launch_sweep16<2, true>(a, nwg, s);
    else if (M == 3) launch_sweep16<3, true>(a, nwg, s);
    else launch_sweep16x2<true>(a, nwg, s);            // paired waves: two tables per wave, 8 waves per workgroup
    fold_slots(gamma, M, s);
    SGA_CHECK_LAUNCH("sga_loss_multi_grad");
    return SGA_OK;
}
extern "C" int sga_loss_multi_grad(const float* const* Z, int M, int D, const float* beta, int A, int J1, int J2, float tau0,
                                   float tau1, const double* gs, float* const* dZ, double* gamma, int a_lo, int a_hi,
                                   void* stream) {
    return multi_grad_impl(Z, M, D, false, beta, A, J1, J2, tau0, tau1, gs, dZ, gamma, a_lo, a_hi, stream);
}
extern "C" int sga_loss_multi_grad_centred(const float* const* Zc, int M, const float* beta, int A, int J1, int J2, float tau0,
                                           float tau1, const double* gs, float* const* dZ, double* gamma, int a_lo, int a_hi,
                                           void* stream) {
    return multi_grad_impl(Zc, M, 102, true, beta, A, J1, J2, tau0, tau1, gs, dZ, gamma, a_lo, a_hi, stream);
}

extern "C" int sga_loss_check_norms(const float* nrm, int n, float* poison, void* stream) {
    SGA_CHECK_ARG(nrm && poison && n >= 0, "sga_loss_check_norms: bad argument");
    if (n == 0) return SGA_OK;
    hipLaunchKernelGGL(check_norms_kernel, dim3(64), dim3(256), 0, static_cast<hipStream_t>(stream), nrm, n, poison);
    SGA_CHECK_LAUNCH("sga_loss_check_norms");
    return SGA_OK;
}

extern "C" int sga_loss_slots(void) { return SGA_SLOTS; }
