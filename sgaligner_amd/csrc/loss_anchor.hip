// Fused anchors x anchors pass of the contrastive / alignment loss (contrastive.hip describes the loss) for the "joint = fusion of the M
// tables" case, M = 2..4, Dp == 104: the forward terms, and the backward that writes the dL/dS stashes, dL/d(sums) and dL/dbeta, in its
// ordered and symmetric (every unordered pair once) forms; the stash products run on gemm.hip.  Every fused step of every MFMA mode ends here.
#include "mfma_tiles.h"
#include <type_traits>

#include "loss_math.h"
#include "aa_launch.h"        // AnchorMultiArgs, inv_sums_kernel, the backward epilogue and its host path (shared with anchor3.hip)

// gemm.hip (include/sgaligner_hip.h): the stash gradient of the anchors x anchors backward runs on the GEMM kernels
extern "C" int sga_gemm(int transA, int transB, int M, int N, int K, const void* A, long lda, int a_is_f64, const float* B,
                        long ldb, float* C, long ldc, const float* bias, int accumulate, void* stream);

namespace {

constexpr int CT_THREADS = 256;
// ------------------------------------------------------------------------------------------------
// Fused anchors x anchors kernel for the "joint = fusion of the M tables" case (Dp == 104).
//
// Same math as anchor_kernel, but S_J = sum_m beta_m S_m is derived in registers, so neither the 312-wide joint
// operand nor its dL/dS stash exist: G_m = dL/dS_m + beta_m dL/dS_J is written directly, and Gamma_m = sum dL/dS_J S_m
// (dL/dbeta) is accumulated on the side.  Geometry, chosen from the counters of anchor_kernel (49 % of wave time in
// waitcnt/barrier on single-buffered K-chunk staging, 512 registers -> 1 wave/SIMD):
//   * a workgroup owns 32 anchor rows I for ALL its J tiles: X1_I / X2_I of the M tables (2*M*13 KiB) are staged into
//     LDS once and are the MFMA B operands (ds_read_b128), so "lane = anchor row i";
//   * each of the 4 waves walks its own 32-row J tiles; the J-side operands go straight from global/L2 into MFMA
//     A-operand fragments (one float4 per lane per 4 MFMAs) -- no staging, no barriers in the loop;
//   * all 2*M S tiles of a (I,J) tile stay in registers (96 for M = 3), ~200 VGPRs total -> 2 waves per SIMD, so one
//     wave's transcendental-heavy epilogue overlaps the other's MFMAs / loads.
// ------------------------------------------------------------------------------------------------
template <int M>
__global__ __launch_bounds__(CT_THREADS, M <= 3 ? 2 : 1) void anchor_multi_kernel(AnchorMultiArgs a) {
    constexpr int DP = 104, NQ = 13, NT = M + 1;
    extern __shared__ __attribute__((aligned(16))) float lds[];      // [M][2][32][DP] own rows + inv_s[NT*8]
    float* inv_s = lds + M * 2 * 32 * DP;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5, l31 = lane & 31;
    const int A = a.A, ns = a.i_hi - a.i_lo;
    const int ib = blockIdx.x / a.nsplit, split = blockIdx.x % a.nsplit;
    const int i0 = a.i_lo + ib * 32;
    const int my_i = i0 + l31;
    const bool iv = my_i < a.i_hi;

    // ---- stage the I block (rows past the shard end are clamped; masked in the epilogue)
    for (int e = tid; e < M * 2 * 32 * (DP / 4); e += CT_THREADS) {
        const int c = (e % (DP / 4)) * 4, r = (e / (DP / 4)) % 32, side = (e / (DP / 4) / 32) % 2, m = e / (DP / 4) / 64;
        const int row = min(i0 + r, a.i_hi - 1) + side * A;
        *reinterpret_cast<f32x4*>(lds + ((m * 2 + side) * 32 + r) * DP + c) = *reinterpret_cast<const f32x4*>(a.Z[m] + (size_t)row * DP + c);
    }
    for (int e = tid; e < NT * 8; e += CT_THREADS) inv_s[e] = (float)(1.0 / (a.sums[e] + 1e-9));
    __syncthreads();
    float beta[M];
#pragma unroll
    for (int m = 0; m < M; ++m) beta[m] = a.beta[m];

    // per-lane partial sums: fp32 within a tile (16 elements), fp64 across this wave's tiles.  (All-fp32 partials lost 1.7e-4 of the IAL
    // terms at configs[2] -- 19 456 nearly equal addends per lane round with a bias, not a random walk; tools/dbg/aa_check64.py.)
    double acc_d[NT + 2 * M];
#pragma unroll
    for (int e = 0; e < NT + 2 * M; ++e) acc_d[e] = 0.0;

    const int ntile = (A + 31) / 32;
    for (int jt = split * 4 + wave; jt < ntile; jt += a.nsplit * 4) {
        const int j0 = jt * 32;
        float acc_out[NT + 2 * M];
#pragma unroll
        for (int e = 0; e < NT + 2 * M; ++e) acc_out[e] = 0.f;
        const int jrow = min(j0 + l31, A - 1);                       // this lane's J row as an MFMA A-operand row
        // ---- S tiles: P[m][r] = S_m[i = lane, j = j0 + row(r,h)],  Q[m][r] = S_m[j, i]
        f32x16 P[M], Q[M];
        zero_acc<M>(P);
        zero_acc<M>(Q);
#pragma unroll
        for (int m = 0; m < M; ++m) {
            const float* gp = a.Z[m] + (size_t)(A + jrow) * DP + 4 * h;      // X2[j] for P
            const float* gq = a.Z[m] + (size_t)jrow * DP + 4 * h;            // X1[j] for Q
            const float* bp = lds + ((m * 2 + 0) * 32 + l31) * DP + 4 * h;   // X1[i]
            const float* bq = lds + ((m * 2 + 1) * 32 + l31) * DP + 4 * h;   // X2[i]
            // J-side fragments are prefetched exactly one K-group ahead into the other of two register pairs; the
            // sched_barrier per group stops the scheduler from hoisting all 2*13 global loads of the table (spills).
            f32x4 apA = *reinterpret_cast<const f32x4*>(gp), aqA = *reinterpret_cast<const f32x4*>(gq), apB = apA, aqB = aqA;
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                if (q + 1 < NQ) {
                    if (q & 1) { apA = *reinterpret_cast<const f32x4*>(gp + 8 * (q + 1)); aqA = *reinterpret_cast<const f32x4*>(gq + 8 * (q + 1)); }
                    else { apB = *reinterpret_cast<const f32x4*>(gp + 8 * (q + 1)); aqB = *reinterpret_cast<const f32x4*>(gq + 8 * (q + 1)); }
                }
                const f32x4 b1 = *reinterpret_cast<const f32x4*>(bp + 8 * q);
                const f32x4 b2 = *reinterpret_cast<const f32x4*>(bq + 8 * q);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    P[m] = __builtin_amdgcn_mfma_f32_32x32x2f32((q & 1) ? apB[r] : apA[r], b1[r], P[m], 0, 0, 0);
                    Q[m] = __builtin_amdgcn_mfma_f32_32x32x2f32((q & 1) ? aqB[r] : aqA[r], b2[r], Q[m], 0, 0, 0);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        // From here on the S tiles are handled as SCALARS: in-place element updates of the 16-wide accumulator vectors
        // (Q[m][r] = ...) make hipcc keep several versions of each vector alive -- >6 KB of scratch per lane.
        float xs[M][16], ys[M][16];
#pragma unroll
        for (int m = 0; m < M; ++m)
#pragma unroll
            for (int r = 0; r < 16; ++r) { xs[m][r] = P[m][r]; ys[m][r] = Q[m][r]; }
        // ---- epilogue, one element at a time (forward)
        const float* js = inv_s + M * 8;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int j = j0 + mfma32_row(r, h);
            const bool ok = iv && j < A;
            float xj = 0.f, yj = 0.f;
#pragma unroll
            for (int m = 0; m < M; ++m) { xj = fmaf(beta[m], xs[m][r], xj); yj = fmaf(beta[m], ys[m][r], yj); }
            {
                const float dji = fexp2(xj * a.ki);
                const float qma = g_val(dji, js[1], js[3]), qmb = g_val(dji, js[5], js[7]);
                const float lqma = flog(qma), lqmb = flog(qmb);
#pragma unroll
                for (int k = 0; k < NT; ++k) {
                    const float x = k < M ? xs[k < M ? k : 0][r] : xj, y = k < M ? ys[k < M ? k : 0][r] : yj;
                    const float* is = inv_s + k * 8;
                    const float qa = g_val(fexp2(x * a.kc), is[0], is[2]);
                    const float qb = g_val(fexp2(y * a.kc), is[4], is[6]);
                    const float term = -flog(a.alpha * qa + (1.f - a.alpha) * qb);
                    acc_out[k] += ok ? term : 0.f;
                    if (k < M) {
                        const float dm = fexp2(x * a.ki);
                        const float qoa = g_val(dm, is[1], is[3]), qob = g_val(dm, is[5], is[7]);
                        const float ta = __expf(qoa) * (qoa - lqma), tb = __expf(qob) * (qob - lqmb);
                        acc_out[NT + (k < M ? k : 0)] += ok ? ta : 0.f;
                        acc_out[NT + M + (k < M ? k : 0)] += ok ? tb : 0.f;
                    }
                }
            }
#pragma unroll
            for (int e = 0; e < NT + 2 * M; ++e) asm volatile("" : "+v"(acc_out[e]));   // keep the updates out of the loop latch
            __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int e = 0; e < NT + 2 * M; ++e) acc_d[e] += (double)acc_out[e];
    }
    // ---- flush the wave's partial sums into its slot
    const int slot = my_slot();
#pragma unroll
    for (int e = 0; e < NT + 2 * M; ++e) {
        const double v = wave_sum_d(acc_d[e]);
        if (lane == 0 && v != 0.0) atomicAdd(a.out + (NT + 2 * M) * (1 + slot) + e, v);
    }
}

// ------------------------------------------------------------------------------------------------
// Backward of the fused anchors x anchors terms on 16x16x4 MFMA tiles.
// The 32x32 form of this epilogue (16 elements per lane, 4 table-major passes, everything unrolled) is ~25 000
// instructions in one loop body and hipcc's register allocator collapses on it (6 KB/lane of scratch, 50 ms).  With
// v_mfma_f32_16x16x4_f32 a lane holds 4 elements of a 16x16 tile, the J loop stays ROLLED, and the body is 4x smaller:
// no scratch, <= 128 registers.  Same geometry otherwise: 32 anchor rows of all M tables resident in LDS (MFMA B
// operand, "lane & 15 = anchor row"), J-side fragments straight from global/L2, waves = (anchor half, J interleave).
// ------------------------------------------------------------------------------------------------
// RB = anchor rows staged per workgroup: 32 (two wave pairs, each walking its own J tiles) for M <= 3; 16 for M = 4, where 32 rows of
// four tables are 106 KiB of LDS = one workgroup per CU (all four waves then share the 16 rows and split the J tiles four ways).
// TERMS: the same launch also accumulates the forward TERM values (what anchor_multi_kernel<M> returns): the epilogue already holds
// every q they are made of, so a training step whose dL/d(terms) is known at forward time (ops.FusedContrastiveFn one-pass mode) runs the
// A x A similarities once instead of twice.
// SYM (M <= 3, TERMS): every UNORDERED anchor pair is visited once.  The block's rows [i_lo, i_hi) meet the columns j >= i_lo only; in a
// tile right of the block (j >= i_hi) a lane holds x = S[i,j] and y = S[j,i] anyway, so it also produces the mirrored element (j, i) --
// its terms, its sum gradients and its coefficient dL/dS[j,i], which goes to a second stash M2 -- instead of leaving it to the block that
// owns row j.  The ICL halves of the two elements share every exp2 / g() evaluation and both denominators; the IAL halves are
// independent.  Half the MFMAs and J-operand loads, ~0.78 of the VALU work per pair.  Tiles inside the block's own
// column range (the diagonal square) run the ordinary epilogue.
template <int M, bool TERMS = false, int RB = (M <= 3 ? 32 : 16), bool SYM = false>
__global__ __launch_bounds__(CT_THREADS, 2) void anchor_multi_bwd16_kernel(AnchorMultiArgs a) {
    static_assert(!SYM || TERMS, "symmetric mode: one-pass build");
    constexpr int DP = 104, NT = M + 1, NSUB = RB / 16, TW = 4 / NSUB;
    extern __shared__ __attribute__((aligned(16))) float lds[];      // [M][2][RB][DP] own rows
    // The (M+1)*8 sum coefficients and the 3M+1 upstream coefficients are read from global memory at uniform addresses, per element
    // of the epilogue (the compiler re-issues them as vector loads after every stash store: it cannot rule out aliasing).  Measured
    // alternatives, 2048 x 155 648 block: as is 9.50 ms; loaded once before the loop (the compiler turns them into s_loads, 82 SGPRs)
    // 10.43 ms; pinned in SGPRs by readfirstlane 11.05 ms -- two-SGPR-operand VALU forms do not exist on gfx9, so the uniform values
    // cost v_movs in the arithmetic, more than the L1-hit loads they replace (tools/bench_aa.py).  As LDS reads each value cost an
    // address VGPR + a data VGPR and pushed the kernel into scratch.
    const float* __restrict__ inv_s = a.inv;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, l15 = lane & 15;
    const int A = a.A, ns = a.i_hi - a.i_lo;
    const int JH = SYM ? a.j_hi : A;                                 // column end (the symmetric walk of a rank stops where another rank's starts)
    int ib, split, nsp;
    aa_unit(a, ib, split, nsp);
    const int i0 = a.i_lo + ib * RB;
    const int ih = wave % NSUB, tw = wave / NSUB;                    // which 16 anchor rows of the block / which share of the J tiles
    const int my_i = i0 + ih * 16 + l15;
    const bool iv = my_i < a.i_hi;

    for (int e = tid; e < M * 2 * RB * (DP / 4); e += CT_THREADS) {
        const int c = (e % (DP / 4)) * 4, r = (e / (DP / 4)) % RB, side = (e / (DP / 4) / RB) % 2, m = e / (DP / 4) / (2 * RB);
        const int row = min(i0 + r, a.i_hi - 1) + side * A;
        *reinterpret_cast<f32x4*>(lds + ((m * 2 + side) * RB + r) * DP + c) = *reinterpret_cast<const f32x4*>(a.Z[m] + (size_t)row * DP + c);
    }
    __syncthreads();
    float beta[M];
#pragma unroll
    for (int m = 0; m < M; ++m) beta[m] = a.beta[m];

    float acc_gs[NT][8], acc_gam[M];
#pragma unroll
    for (int k = 0; k < NT; ++k)
#pragma unroll
        for (int e = 0; e < 8; ++e) acc_gs[k][e] = 0.f;
#pragma unroll
    for (int m = 0; m < M; ++m) acc_gam[m] = 0.f;
    float acc_out[TERMS ? NT + 2 * M : 1];                           // TERMS: [ICL_0..M | IAL_a 0..M-1 | IAL_b 0..M-1] partial sums
#pragma unroll
    for (int e = 0; e < (TERMS ? NT + 2 * M : 1); ++e) acc_out[e] = 0.f;
    int tiles_done = 0;
    // (the running sums are fp32 per lane and leave for the fp64 slots every 32 tiles: aa_flush)
    const int slot = my_slot();
    auto flush = [&]() { aa_flush<M, TERMS>(a, inv_s, lane, slot, acc_gs, acc_gam, acc_out); };

    const int ntile = (JH + 15) / 16;
#pragma unroll 1
    for (int jt = (a.j_lo >> 4) + split * TW + tw; jt < ntile; jt += nsp * TW) {
        const int j0 = jt * 16;
        const int jrow = min(j0 + l15, A - 1);
        // The anchor-row operands are loop invariant; left alone, LICM parks all M*2*26 of them in registers
        // (156 for M = 3) and the kernel drops to one wave per SIMD with AGPR/scratch spills.  An opaque zero
        // offset keeps the ds_reads inside the loop: ~100 registers, two waves per SIMD hide each other's loads.
        int lofs = 0;
        asm volatile("" : "+v"(lofs));
        f32x4 P[M], Q[M];
        // J-side operands of table m + 1 are requested (all 12 quads + tails) before table m's MFMAs start: a whole table of flight time
        // for loads that come straight from L2 (compiler-scheduled two loads ahead: 12.80 ms per symmetric 2048 x 155 648 block; this: 12.39)
        struct JOps { f32x4 p[6], q[6]; float pt[2], qt[2]; };
        auto jload = [&](int m, JOps& o) {
            const float* gp = a.Z[m] + (size_t)(A + jrow) * DP;              // X2[j] for P
            const float* gq = a.Z[m] + (size_t)jrow * DP;                    // X1[j] for Q
#pragma unroll
            for (int q = 0; q < 6; ++q) {
                o.p[q] = *reinterpret_cast<const f32x4*>(gp + 16 * q + 4 * g);
                o.q[q] = *reinterpret_cast<const f32x4*>(gq + 16 * q + 4 * g);
            }
#pragma unroll
            for (int t = 0; t < 2; ++t) { o.pt[t] = gp[96 + 4 * t + g]; o.qt[t] = gq[96 + 4 * t + g]; }
        };
        constexpr bool JDB = true;        // (M = 4, symmetric: 54 VGPRs go to scratch with or without the second buffer -- cold values, 2 reloads per element)
        JOps jb[JDB ? 2 : 1];
        jload(0, jb[0]);
#pragma unroll
        for (int m = 0; m < M; ++m) {
            if (JDB) { if (m + 1 < M) jload(m + 1, jb[JDB ? (m + 1) & 1 : 0]); }
            else if (m > 0) jload(m, jb[0]);
            __builtin_amdgcn_sched_barrier(0);
            P[m] = f32x4{0.f, 0.f, 0.f, 0.f};
            Q[m] = P[m];
            const JOps& o = jb[JDB ? m & 1 : 0];
            const float* bp = lds + lofs + ((m * 2 + 0) * RB + ih * 16 + l15) * DP;   // X1[i]
            const float* bq = lds + lofs + ((m * 2 + 1) * RB + ih * 16 + l15) * DP;   // X2[i]
#pragma unroll
            for (int q = 0; q < 6; ++q) {                                    // k = 16q + 4g + r
                const f32x4 b1 = *reinterpret_cast<const f32x4*>(bp + 16 * q + 4 * g);
                const f32x4 b2 = *reinterpret_cast<const f32x4*>(bq + 16 * q + 4 * g);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    P[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(o.p[q][r], b1[r], P[m], 0, 0, 0);
                    Q[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(o.q[q][r], b2[r], Q[m], 0, 0, 0);
                }
            }
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const int kk = 96 + 4 * t + g;
                P[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(o.pt[t], bp[kk], P[m], 0, 0, 0);
                Q[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(o.qt[t], bq[kk], Q[m], 0, 0, 0);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        // P[m][r] = S_m[i = lane&15, j = j0 + 4g + r], Q[m][r] = S_m[j, i]: the epilogue of aa_epilogue.h, one element (r) at a time.  Interior
        // tiles (all 16 anchor rows and all 16 columns valid: everything but the last row block / column tile) run its mask-free form.
        const int jg = j0 + 4 * g;
        if constexpr (SYM) {
            if (j0 >= a.mir) aa_epilogue_sym<M>(a, inv_s, beta, P, Q, acc_gs, acc_gam, acc_out, jg, JH, iv, my_i, ns);                      // uniform
            else aa_epilogue<M, TERMS, true>(a, inv_s, beta, P, Q, acc_gs, acc_gam, acc_out, jg, JH, iv, my_i, ns);
        } else {
            if (j0 + 16 <= A && i0 + RB <= a.i_hi) aa_epilogue<M, TERMS, false>(a, inv_s, beta, P, Q, acc_gs, acc_gam, acc_out, jg, JH, iv, my_i, ns);   // uniform
            else aa_epilogue<M, TERMS, true>(a, inv_s, beta, P, Q, acc_gs, acc_gam, acc_out, jg, JH, iv, my_i, ns);
        }
        if ((++tiles_done & (SYM ? 15 : 31)) == 0) flush();          // uniform
    }
    flush();
}

}  // namespace

// ---- fused anchors x anchors entry points -------------------------------------------------------------------------
extern "C" int sga_loss_anchor_multi_fwd(const float* const* Z, int M, const float* beta, int A, const double* sums,
                                         float alpha, float tau_icl, float tau_ial, double* out, int a_lo, int a_hi,
                                         void* stream) {
    SGA_CHECK_ARG(Z && beta && sums && out && A >= 0, "sga_loss_anchor_multi_fwd: bad argument");
    SGA_CHECK_ARG(M >= 2 && M <= 4, "sga_loss_anchor_multi_fwd: M=%d not in {2,3,4} (use the per-table kernels)", M);
    SGA_CHECK_ARG(a_lo >= 0 && a_hi <= A && a_lo <= a_hi, "sga_loss_anchor_multi_fwd: anchor shard [%d,%d) outside [0,%d]", a_lo, a_hi, A);
    for (int m = 0; m < M; ++m) SGA_CHECK_ARG(Z[m], "sga_loss_anchor_multi_fwd: null table");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int n = (M + 1) + 2 * M;
    if (int rc0 = zero_slots(out, n, s, "sga_loss_anchor_multi_fwd")) return rc0;
    if (A == 0 || a_hi <= a_lo) return SGA_OK;
    AnchorMultiArgs a{};
    aa_fill(a, M, beta, A, sums, alpha, tau_icl, tau_ial, a_lo, a_hi);
    for (int m = 0; m < M; ++m) a.Z[m] = Z[m];
    a.out = out;
    // 32 anchor rows per workgroup, whose four waves walk 32-row J tiles side by side: one split count for all row blocks, searched from
    // ~4 rounds of workgroups up (aa_plan without its second run).  Timed against the split count it had, ceil(4 CUs / row blocks), for
    // M = 2, 3, 4 and A = 992 .. 38 912 (profiles/aa_fill_forward.txt): equal or faster (M = 3, A = 38 912: 25.2 -> 22.9 ms) except
    // M = 2, A = 4096, 0.230 -> 0.262 ms.
    const int nib = (a_hi - a_lo + 31) / 32;
    const size_t lds = (size_t)(M * 2 * 32 * 104 + (M + 1) * 8) * sizeof(float);
    auto k = M == 2 ? anchor_multi_kernel<2> : M == 3 ? anchor_multi_kernel<3> : anchor_multi_kernel<4>;
    hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    a.nsplit = aa_plan(nib, (A + 31) / 32, 4, aa_slots(reinterpret_cast<const void*>(k), CT_THREADS, lds), 4, false).n1;
    hipLaunchKernelGGL(k, dim3(nib * a.nsplit), dim3(CT_THREADS), lds, s, a);
    fold_slots(out, n, s);
    SGA_CHECK_LAUNCH("sga_loss_anchor_multi_fwd");
    return SGA_OK;
}

// The backward entry points (aa_launch.h): RB anchor rows per workgroup and 4 * 16 / RB shares of the 16-column J tiles; ~6 rounds of workgroups.
template <int M>
static AAKernels<AnchorMultiArgs> anchor_multi_bwd_kernels() {
    constexpr int RB = M <= 3 ? 32 : 16;                             // (the kernel's own default)
    static_assert(aa_geom(false, M).rows == RB && aa_geom(false, M).shares == 64 / RB, "the plan's numbers are this kernel's");
    return {anchor_multi_bwd16_kernel<M, true, RB, true>, anchor_multi_bwd16_kernel<M, true>, anchor_multi_bwd16_kernel<M, false>, aa_geom(false, M),
            (size_t)(M * 2 * RB * 104 + (M + 1) * 8) * sizeof(float)};
}

static int anchor_multi_bwd(const AAContract& c, const AAOperands& o, const float* const* Z, void* stream) {
    if (int rc = aa_validate(c, o)) return rc;
    AnchorMultiArgs a{};
    for (int m = 0; m < o.M; ++m) a.Z[m] = Z[m];
    const auto kern = o.M == 2 ? anchor_multi_bwd_kernels<2>() : o.M == 3 ? anchor_multi_bwd_kernels<3>() : anchor_multi_bwd_kernels<4>();
    return aa_run(c, o, a, a, kern, CT_THREADS, stream);
}

/* The launch plan of an A x A backward job (aa_launch.h: aa_plan) on `slots` workgroup slots, nothing launched and no device asked.
 * planes != 0: sga_loss_anchor_multi_bwd_symx_bf16x6, else the fp32 entry points.  plan[8] = {rows of a row block, 16-column halves a
 * workgroup walks side by side per step, row blocks, row blocks of the first run, splits of a row block in the first run, splits in the
 * second, workgroups, steps of a row block}.  Workgroup w < nib1 * n1 is (row block w / n1, split w % n1 of n1), the others likewise
 * behind them with n2; split s of n walks the steps s, s + n, ... */
extern "C" int sga_loss_anchor_plan(int planes, int M, int A, int a_lo, int a_hi, int j_lo, int j_hi, int slots, int32_t* plan) {
    SGA_CHECK_ARG(plan && slots >= 1 && M >= 2 && M <= (planes ? 3 : 4) && A >= 0 && a_lo >= 0 && a_lo <= a_hi && a_hi <= A && j_lo >= 0 && j_lo <= j_hi &&
                      j_hi <= A && j_lo % 16 == 0, "sga_loss_anchor_plan: bad argument");
    const AAGeom g = aa_geom(planes != 0, M);
    const AAPlan p = aa_job_plan(g, a_lo, a_hi, j_lo, j_hi, slots);
    const int nib = (a_hi - a_lo + g.rows - 1) / g.rows, ntile16 = ((j_hi + g.col_tile - 1) / g.col_tile * g.col_tile - j_lo) / 16;
    const int32_t out[8] = {g.rows, g.shares, nib, p.nib1, p.n1, p.n2, j_hi > j_lo ? p.wgs : 0, (ntile16 + g.shares - 1) / g.shares};
    for (int i = 0; i < 8; ++i) plan[i] = out[i];
    return SGA_OK;
}

extern "C" int sga_loss_anchor_multi_bwd(const float* const* Z, int M, const float* beta, int A, const double* sums,
                                         float alpha, float tau_icl, float tau_ial, const float* coef, float* const* M1,
                                         double* gs, double* gamma, int a_lo, int a_hi, double* out_terms, void* stream) {
    static const AAContract C = {"sga_loss_anchor_multi_bwd", 2, 4, 1, 16, AA_ORDERED};
    return anchor_multi_bwd(C, {reinterpret_cast<const void* const*>(Z), M, beta, A, sums, alpha, tau_icl, tau_ial, coef, M1, nullptr, gs, gamma,
                                a_lo, a_hi, 0, A, A, out_terms}, Z, stream);
}

/* Symmetric form of sga_loss_anchor_multi_bwd (terms always returned; jobs and stash layouts: include/sgaligner_hip.h): rows [a_lo, a_hi) meet
 * the columns [j_lo, j_hi) only, tiles at j >= mir also produce the mirrored elements (j, i) into M2, tiles left of mir are visited in the
 * ordered way.  An unsharded anchor set walked in blocks is (j_lo, j_hi, mir) = (a_lo, A, a_hi): every unordered pair once over the walk. */
extern "C" int sga_loss_anchor_multi_bwd_symx(const float* const* Z, int M, const float* beta, int A, const double* sums, float alpha,
                                              float tau_icl, float tau_ial, const float* coef, float* const* M1, float* const* M2,
                                              double* gs, double* gamma, int a_lo, int a_hi, int j_lo, int j_hi, int mir, double* out_terms,
                                              void* stream) {
    static const AAContract C = {"sga_loss_anchor_multi_bwd_symx", 2, 4, 32, 16, AA_SYMMETRIC};
    return anchor_multi_bwd(C, {reinterpret_cast<const void* const*>(Z), M, beta, A, sums, alpha, tau_icl, tau_ial, coef, M1, M2, gs, gamma,
                                a_lo, a_hi, j_lo, j_hi, mir, out_terms}, Z, stream);
}

/* The four products of a symmetric block's two stashes for one table (Z = [X1 | X2 | ...] rows of width Dp; R = [a_lo, a_hi), C = [j_lo, j_hi),
 * C' = [mir, j_hi)):    dX1[R] += M1^T X2[C]     dX2[C] += M1 X1[R]     dX1[C'] += M2 X2[R]     dX2[R] += M2^T X1[C'] */
extern "C" int sga_loss_stash_grad_symx(const float* M1, const float* M2, const float* Z, int A, int Dp, float* dZ, int a_lo, int a_hi,
                                        int j_lo, int j_hi, int mir, void* stream) {
    SGA_CHECK_ARG(M1 && Z && dZ && A >= 0 && Dp >= 8 && Dp % 8 == 0 && a_lo >= 0 && a_hi <= A && a_lo <= a_hi && j_lo >= 0 && j_lo <= j_hi && j_hi <= A &&
                  mir >= j_lo && (M2 || mir >= j_hi), "sga_loss_stash_grad_symx: bad argument");
    const int ns = a_hi - a_lo, c1 = j_hi - j_lo, c2 = mir < j_hi ? j_hi - mir : 0;
    if (A == 0 || ns == 0 || c1 == 0) return SGA_OK;
    // (a last block whose row count is not a multiple of 4 takes sga_gemm's general kernel: correct, slower)
    const float* X1 = Z;
    const float* X2 = Z + (size_t)A * Dp;
    float* d1 = dZ;
    float* d2 = dZ + (size_t)A * Dp;
    int rc = sga_gemm(1, 0, ns, Dp, c1, M1, ns, 0, X2 + (size_t)j_lo * Dp, Dp, d1 + (size_t)a_lo * Dp, Dp, nullptr, 1, stream);
    if (!rc) rc = sga_gemm(0, 0, c1, Dp, ns, M1, ns, 0, X1 + (size_t)a_lo * Dp, Dp, d2 + (size_t)j_lo * Dp, Dp, nullptr, 1, stream);
    if (!rc && c2 > 0) rc = sga_gemm(0, 0, c2, Dp, ns, M2, ns, 0, X2 + (size_t)a_lo * Dp, Dp, d1 + (size_t)mir * Dp, Dp, nullptr, 1, stream);
    if (!rc && c2 > 0) rc = sga_gemm(1, 0, ns, Dp, c2, M2, ns, 0, X1 + (size_t)mir * Dp, Dp, d2 + (size_t)a_lo * Dp, Dp, nullptr, 1, stream);
    return rc;
}
