// The anchors x anchors backward (loss_anchor.hip: anchor_multi_bwd16_kernel) with its similarities formed on the bf16 matrix pipe from the
// three-plane image the sweeps already use (sweep3.hip, sga_loss_split3_tables), M = 2, 3.  Everything behind the similarities -- the joint
// S, the g() evaluations, the terms, the transposed coefficient stashes, the partial sums, the masks, the mirrored element -- is the fp32
// kernel's own epilogue (aa_epilogue.h).
//
// A similarity is the sweeps' sub-step: per table and side 20 v_mfma_f32_16x16x32_bf16 in ONE fp32 accumulator chain, in the sweeps' order
//     tails (O1, O0) | l h | m m | m h | h l | h m | h h          (J row's plane x own row's plane),
// the K tail on two K = 32 MFMAs against the tail image; the own side holds (1, b_i) against the image's (b_j, 1), so the chain delivers
// z_i . z_j of the centred rows.  640 matrix cycles per 16 x 16 tile and table where the fp32 kernel issues 2 x 26 v_mfma_f32_16x16x4_f32
// (1664 cycles, on the datapath the epilogue's VALU work needs too).
//
// Geometry.  A workgroup of 8 waves owns 32 anchor rows I for all its J tiles.  Prologue: rows X1[I], X2[I] of the M tables go from the image
// to LDS as the MFMA B operand IN OPERAND ORDER -- per (table, side, 16-row half) 11 operands (the two tail operands, tail swap done here,
// then 3 planes x 3 K steps) of 64 lanes x 16 B, read back lane-linear by ds_read_b128: 11 KiB x 2 halves x 2 sides x M = 132 KiB for M = 3,
// one workgroup per CU, two waves per SIMD.  No barrier in the J loop.  Waves = (anchor half ih, J share tw of 4): a wave's tile is 16 own rows
// x one 16-row half (jb, jh) of a 32-row image block, whose A-operand fragments come straight from the image in global memory / L2, 16 B per
// lane at the sweeps' slot of the lane (lane-linear up to the bank swizzle): 10 loads per sub-step, requested one sub-step ahead.  The two
// waves that share a J share read the same fragments (L1).  Row map of a half: operand row i <-> block row 8 (i >> 2) + 4 jh + (i & 3), so a
// lane's four accumulator values are the columns 32 jb + 8 g + 4 jh + r; with a_lo, j_lo, mir on 32-row boundaries every image block is
// uniformly diagonal-square, ordered or mirrored.
#include "mfma_tiles.h"
#include <type_traits>

#include "s3_layout.h"
#include "aa_epilogue.h"

namespace {

constexpr int A3_THREADS = 512;
constexpr int A3_TW = 4;                          // J shares per workgroup (waves = 2 anchor halves x A3_TW)
constexpr int A3_NOP = 11;                        // own operands per (table, side, half): O1, O0, then [plane h, m, l][K step]

struct Anchor3Args {
    AnchorMultiArgs a;                            // (Z unused)
    const unsigned char* Zb[4];                   // the tables' three-plane images
    int nbA;                                      // blocks of the X1 segment: X2's block b is image block nbA + b
};

__device__ __forceinline__ u32x4 a3_ld(const unsigned char* p) { return *reinterpret_cast<const u32x4*>(p); }

template <int M, bool TERMS, bool SYM>
__global__ __launch_bounds__(A3_THREADS) void anchor3_bwd_kernel(Anchor3Args A3) {
    static_assert(!SYM || TERMS, "symmetric mode: one-pass build");
    static_assert(M == 2 || M == 3, "two or three tables");
    const AnchorMultiArgs& a = A3.a;
    extern __shared__ __attribute__((aligned(16))) u32x4 own3[];      // [M][side 2][half 2][A3_NOP][64 lanes]
    const float* __restrict__ inv_s = a.inv;                          // (read per element from global memory: see anchor_multi_bwd16_kernel)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, l15 = lane & 15;
    const int A = a.A, ns = a.i_hi - a.i_lo;
    const int JH = SYM ? a.j_hi : A;
    const int ib = blockIdx.x / a.nsplit, split = blockIdx.x % a.nsplit;
    const int i0 = a.i_lo + ib * 32;                                  // a multiple of 32: image block i0 >> 5 of both anchor segments
    const int ih = wave & 1, tw = wave >> 1;
    const int my_i = i0 + ih * 16 + l15;
    const bool iv = my_i < a.i_hi;                                    // (rows past the end are the image's zero padding rows: S = 0, masked)

    // ---- prologue: the block's own rows as B operands, in operand order
    if (tid < 256) {
        const int ln = tid & 63, hh = (tid >> 6) & 1, side = tid >> 7;
        const int gg = ln >> 4, o = hh * 16 + (ln & 15);
        const int ojh = (o >> 2) & 1, oi = 4 * (o >> 3) + (o & 3);   // block row o sits at (half ojh, operand row oi)
        const int so = (ojh * 64 + s3_slot(gg, oi)) * 16;
#pragma unroll
        for (int m = 0; m < M; ++m) {
            const unsigned char* base = A3.Zb[m] + (size_t)(side * A3.nbA + (i0 >> 5)) * S3_BLOCK;
            u32x4* dst = own3 + (((m * 2 + side) * 2 + hh) * A3_NOP) * 64 + ln;
            const unsigned char* tb = base + S3_TAIL + ojh * 1024;
            const u32x4 th = a3_ld(tb + s3_slot(0, oi) * 16), tm = a3_ld(tb + s3_slot(2, oi) * 16), tl = a3_ld(tb + s3_slot(3, oi) * 16);
            u32x4 ot[2];                                                  // O0 = (h, m, h, h), O1 = (l, 0, m, 0); the chain starts with O1
            s3_own_tails(th, tm, tl, gg, ot);
            dst[0] = ot[1];
            dst[64] = ot[0];
#pragma unroll
            for (int p = 0; p < 3; ++p)
#pragma unroll
                for (int q = 0; q < 3; ++q) dst[(2 + p * 3 + q) * 64] = a3_ld(base + p * S3_PLANE + q * 2048 + so);
        }
    }
    __syncthreads();
    float beta[M];
#pragma unroll
    for (int m = 0; m < M; ++m) beta[m] = a.beta[m];

    constexpr int NT = M + 1;
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
    const int slot = my_slot();

    const int aoff = s3_slot(g, l15) * 16;                           // the lane's slot in a [64 slots][16 B] operand image
    const int jt_end = 2 * ((JH + 31) >> 5);                         // 16-row halves: jt = 2 jb + jh
#pragma unroll 1
    for (int jt = (a.j_lo >> 4) + split * A3_TW + tw; jt < jt_end; jt += a.nsplit * A3_TW) {
        const int jb = jt >> 1, jh = jt & 1, j0 = 32 * jb;
        // The own operands are loop invariant; an opaque zero offset keeps their ds_reads inside the loop (as in anchor_multi_bwd16_kernel:
        // hoisted they would take 2 M x 44 registers).
        int lofs = 0;
        asm volatile("" : "+v"(lofs));
        f32x4 P[M], Q[M];
        // sub-step ss = (table ss >> 1, side ss & 1): side 0 is P = X1[i] . X2[j] (J rows from the X2 segment), side 1 is Q = X1[j] . X2[i]
        struct JF { u32x4 t, p[3][3]; };
        auto jload = [&](int ss, JF& o) {
            const unsigned char* ar = A3.Zb[ss >> 1] + (size_t)(((ss & 1) ? 0 : A3.nbA) + jb) * S3_BLOCK + jh * 1024 + aoff;
            o.t = a3_ld(ar + S3_TAIL);
#pragma unroll
            for (int p = 0; p < 3; ++p)
#pragma unroll
                for (int q = 0; q < 3; ++q) o.p[p][q] = a3_ld(ar + p * S3_PLANE + q * 2048);
        };
        JF jf[2];
        jload(0, jf[0]);
#pragma unroll
        for (int ss = 0; ss < 2 * M; ++ss) {
            if (ss + 1 < 2 * M) jload(ss + 1, jf[(ss + 1) & 1]);    // a whole sub-step of flight time
            __builtin_amdgcn_sched_barrier(0);
            const JF& o = jf[ss & 1];
            const u32x4* bo = own3 + lofs + ((ss * 2 + ih) * A3_NOP) * 64 + lane;
            u32x4 ow[A3_NOP];
#pragma unroll
            for (int k = 0; k < A3_NOP; ++k) ow[k] = bo[k * 64];
            constexpr int PA[6] = {2, 1, 1, 0, 0, 0}, PB[6] = {0, 1, 0, 2, 1, 0};
            f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
            acc = mfma_b(o.t, ow[0], acc);
            acc = mfma_b(o.t, ow[1], acc);
#pragma unroll
            for (int x = 0; x < 6; ++x)
#pragma unroll
                for (int q = 0; q < 3; ++q) acc = mfma_b(o.p[PA[x]][q], ow[2 + PB[x] * 3 + q], acc);
            if (ss & 1) Q[ss >> 1] = acc; else P[ss >> 1] = acc;
            __builtin_amdgcn_sched_barrier(0);
        }
        // P[m][r] = S_m[i = my_i, j = jg + r], Q[m][r] = S_m[j, i]
        const int jg = j0 + 8 * g + 4 * jh;
        if constexpr (SYM) {
            if (j0 >= a.mir) aa_epilogue_sym<M>(a, inv_s, beta, P, Q, acc_gs, acc_gam, acc_out, jg, JH, iv, my_i, ns);                     // uniform
            else aa_epilogue<M, TERMS, true>(a, inv_s, beta, P, Q, acc_gs, acc_gam, acc_out, jg, JH, iv, my_i, ns);
        } else {
            if (j0 + 32 <= A && i0 + 32 <= a.i_hi) aa_epilogue<M, TERMS, false>(a, inv_s, beta, P, Q, acc_gs, acc_gam, acc_out, jg, JH, iv, my_i, ns);   // uniform
            else aa_epilogue<M, TERMS, true>(a, inv_s, beta, P, Q, acc_gs, acc_gam, acc_out, jg, JH, iv, my_i, ns);
        }
        if ((++tiles_done & (SYM ? 15 : 31)) == 0) aa_flush<M, TERMS>(a, inv_s, lane, slot, acc_gs, acc_gam, acc_out);                    // uniform
    }
    aa_flush<M, TERMS>(a, inv_s, lane, slot, acc_gs, acc_gam, acc_out);
}

}  // namespace

/* sga_loss_anchor_multi_bwd_symx on the three-plane images Zb[m] (sga_loss_split3_tables with the same A, J1, J2), M = 2, 3: same outputs, same
 * stash layouts, same gs / gamma / out_terms slots and fold.  The ordered walk of a block is (j_lo, j_hi, mir) = (0, A, A) with M2 == NULL
 * (out_terms may then be NULL: no term values).  a_lo, j_lo, mir: multiples of 32 (mir >= j_hi: no mirrored elements); a_hi, j_hi: multiples
 * of 32 or == A. */
extern "C" int sga_loss_anchor_multi_bwd_symx_bf16x6(const void* const* Zb, int M, const float* beta, int A, int J1, int J2, const double* sums,
                                                     float alpha, float tau_icl, float tau_ial, const float* coef, float* const* M1, float* const* M2,
                                                     double* gs, double* gamma, int a_lo, int a_hi, int j_lo, int j_hi, int mir, double* out_terms,
                                                     void* stream) {
    SGA_CHECK_ARG(Zb && beta && sums && coef && M1 && gs && gamma && A >= 0 && J1 >= 0 && J2 >= 0, "sga_loss_anchor_multi_bwd_symx_bf16x6: bad argument");
    SGA_CHECK_ARG(M == 2 || M == 3, "sga_loss_anchor_multi_bwd_symx_bf16x6: M=%d (2 or 3; four tables take sga_loss_anchor_multi_bwd_symx)", M);
    SGA_CHECK_ARG(a_lo >= 0 && a_lo <= a_hi && a_hi <= A && a_lo % 32 == 0 && (a_hi % 32 == 0 || a_hi == A),
                  "sga_loss_anchor_multi_bwd_symx_bf16x6: block [%d,%d) not on 32-row boundaries of [0,%d]", a_lo, a_hi, A);
    SGA_CHECK_ARG(j_lo >= 0 && j_lo % 32 == 0 && j_hi <= A && j_lo <= j_hi && (j_hi % 32 == 0 || j_hi == A) && mir >= j_lo && (mir % 32 == 0 || mir >= j_hi),
                  "sga_loss_anchor_multi_bwd_symx_bf16x6: columns [%d,%d) / mirror start %d not on 32-column boundaries", j_lo, j_hi, mir);
    // columns left of the mirror start are visited in the ordered way: the whole ordered walk (0, A, A), or columns of the block's own square
    const bool ordered = j_lo == 0 && j_hi == A && mir >= j_hi;
    SGA_CHECK_ARG(ordered || mir <= j_lo || (j_lo >= a_lo && (mir < j_hi ? mir : j_hi) <= a_hi),
                  "sga_loss_anchor_multi_bwd_symx_bf16x6: ordered columns [%d,%d) outside the block's square [%d,%d)", j_lo, mir, a_lo, a_hi);
    SGA_CHECK_ARG(ordered || out_terms, "sga_loss_anchor_multi_bwd_symx_bf16x6: a symmetric launch returns its terms (out_terms == NULL)");
    for (int m = 0; m < M; ++m)
        SGA_CHECK_ARG(Zb[m] && M1[m] && (mir >= j_hi || (M2 && M2[m])), "sga_loss_anchor_multi_bwd_symx_bf16x6: null table or stash");
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (int rc0 = zero_slots(gs, (M + 1) * 8, s, "sga_loss_anchor_multi_bwd_symx_bf16x6")) return rc0;
    if (int rc1 = zero_slots(gamma, M, s, "sga_loss_anchor_multi_bwd_symx_bf16x6")) return rc1;
    if (out_terms) { if (int rc2 = zero_slots(out_terms, (M + 1) + 2 * M, s, "sga_loss_anchor_multi_bwd_symx_bf16x6")) return rc2; }
    if (A == 0 || a_hi <= a_lo || j_hi <= j_lo) return SGA_OK;
    Anchor3Args k{};
    AnchorMultiArgs& a = k.a;
    a.M = M; a.A = A; a.i_lo = a_lo; a.i_hi = a_hi; a.beta = beta; a.sums = sums; a.alpha = alpha;
    a.kc = LOG2E / tau_icl; a.ki = LOG2E / tau_ial; a.itc = 1.f / tau_icl; a.iti = 1.f / tau_ial;
    a.coef = coef; a.gs = gs; a.gamma = gamma; a.out = out_terms;
    a.j_lo = j_lo; a.j_hi = j_hi; a.mir = mir;
    k.nbA = make_tlayout(A, J1, J2).nbA;
    for (int m = 0; m < M; ++m) {
        k.Zb[m] = static_cast<const unsigned char*>(Zb[m]);
        a.M1[m] = M1[m]; a.M2[m] = M2 ? M2[m] : nullptr;
    }
    // float copy of 1/(sums+eps): lives in the block after the gs slots (gs buffers hold (2 + slots) * (M+1)*8 doubles)
    float* inv = reinterpret_cast<float*>(gs + (size_t)(1 + SGA_SLOTS) * (M + 1) * 8);
    hipLaunchKernelGGL(inv_sums_kernel, dim3(1), dim3(64), 0, s, sums, inv, (M + 1) * 8);
    a.inv = inv;
    // one workgroup per CU (LDS): ~3 rounds of workgroups, each with at least one tile per wave
    const size_t lds = (size_t)M * 2 * 2 * A3_NOP * 1024;
    const int nib = (a_hi - a_lo + 31) / 32, ntile16 = 2 * ((j_hi + 31) / 32) - (j_lo >> 4);
    int nsp = (3 * sga_num_cus() + nib - 1) / nib;
    if (nsp > (ntile16 + A3_TW - 1) / A3_TW) nsp = (ntile16 + A3_TW - 1) / A3_TW;
    if (nsp < 1) nsp = 1;
    a.nsplit = nsp;
    auto go = [&](auto kern) {
        hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        hipLaunchKernelGGL(kern, dim3(nib * nsp), dim3(A3_THREADS), lds, s, k);
    };
    if (!ordered) { if (M == 2) go(anchor3_bwd_kernel<2, true, true>); else go(anchor3_bwd_kernel<3, true, true>); }
    else if (out_terms) { if (M == 2) go(anchor3_bwd_kernel<2, true, false>); else go(anchor3_bwd_kernel<3, true, false>); }
    else { if (M == 2) go(anchor3_bwd_kernel<2, false, false>); else go(anchor3_bwd_kernel<3, false, false>); }
    if (out_terms) fold_slots(out_terms, (M + 1) + 2 * M, s);
    fold_slots(gs, (M + 1) * 8, s);
    fold_slots(gamma, M, s);
    SGA_CHECK_LAUNCH("sga_loss_anchor_multi_bwd_symx_bf16x6");
    return SGA_OK;
}
