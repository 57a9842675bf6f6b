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
#include "aa_launch.h"

namespace {

constexpr int A3_THREADS = 512;
constexpr int A3_TW = 4;                          // J shares per workgroup (waves = 2 anchor halves x A3_TW)
constexpr int A3_NOP = 11;                        // own operands per (table, side, half): O1, O0, then [plane h, m, l][K step]
constexpr size_t a3_lds_bytes(int M) { return (size_t)M * 2 * 2 * A3_NOP * 1024; }      // the workgroup's own rows: what the launch asks for
static_assert(a3_lds_bytes(3) <= 160 * 1024, "the own rows of three tables fit a CU's LDS");

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
    int ib, split, nsp;
    aa_unit(a, ib, split, nsp);
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
    for (int jt = (a.j_lo >> 4) + split * A3_TW + tw; jt < jt_end; jt += nsp * A3_TW) {
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

template <int M>
AAKernels<Anchor3Args> anchor3_kernels() {
    static_assert(aa_geom(true, M).rows == 32 && aa_geom(true, M).shares == A3_TW, "the plan's numbers are this kernel's");
    return {anchor3_bwd_kernel<M, true, true>, anchor3_bwd_kernel<M, true, false>, anchor3_bwd_kernel<M, false, false>, aa_geom(true, M), a3_lds_bytes(M)};
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
    // (four tables take sga_loss_anchor_multi_bwd_symx)
    static const AAContract C = {"sga_loss_anchor_multi_bwd_symx_bf16x6", 2, 3, 32, 32, AA_EITHER};
    const AAOperands o = {Zb, M, beta, A, sums, alpha, tau_icl, tau_ial, coef, M1, M2, gs, gamma, a_lo, a_hi, j_lo, j_hi, mir, out_terms};
    SGA_CHECK_ARG(J1 >= 0 && J2 >= 0, "sga_loss_anchor_multi_bwd_symx_bf16x6: bad argument");
    if (int rc = aa_validate(C, o)) return rc;
    Anchor3Args k{};
    k.nbA = make_tlayout(A, J1, J2).nbA;
    for (int m = 0; m < M; ++m) k.Zb[m] = static_cast<const unsigned char*>(Zb[m]);
    // 32 anchor rows per workgroup, one workgroup per CU (LDS); how the row blocks are cut into workgroups: aa_plan
    return aa_run(C, o, k, k.a, M == 2 ? anchor3_kernels<2>() : anchor3_kernels<3>(), A3_THREADS, stream);
}
