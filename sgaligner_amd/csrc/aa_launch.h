// The host side of the anchors x anchors backward, once for every kernel that ends in aa_epilogue.h (loss_anchor.hip: fp32 MFMA over the
// packed tables; anchor3.hip: bf16 MFMA over the three-plane image): what an entry point accepts (AAContract), the checks of a job against
// it (aa_validate), the split plan (aa_plan) and everything from the zeroing of the slots to the folds (aa_run).  An entry point is its
// contract, its kernels (AAKernels) with their LDS size and grid numbers, the table pointers in its kernel's own argument struct, one call.
#pragma once
#include "aa_epilogue.h"

namespace {

enum AAWalk {
    AA_ORDERED,        // the ordered block (j_lo, j_hi, mir) = (0, A, A), nothing else (the entry point builds the job itself)
    AA_SYMMETRIC,      // every job runs the symmetric kernel, (0, A, A) too
    AA_EITHER          // (0, A, A) runs the ordered kernels, every other job the symmetric one
};

struct AAContract {
    const char* name;  // the entry point: every message starts with it
    int m_lo, m_hi;    // tables
    int row_align;     // a_lo, and a_hi unless it is A, are multiples of this
    int col_tile;      // j_lo, j_hi unless it is A, and mir unless it is >= j_hi, are multiples of this: the kernel's column tile, 16 or 32
    AAWalk walk;
};

// An entry point's arguments under the names the C ABI gives them (include/sgaligner_hip.h); tables: Z, or the images Zb.
struct AAOperands {
    const void* const* tables;
    int M; const float* beta; int A; const double* sums;
    float alpha, tau_icl, tau_ial;
    const float* coef; float* const* M1; float* const* M2; double *gs, *gamma;
    int a_lo, a_hi, j_lo, j_hi, mir;
    double* out_terms;
};

// One row per table count.  The kernels of a row differ in (SYM, TERMS) only: the symmetric one (always with terms) and the ordered ones
// with and without term values.
template <class KArgs>
struct AAKernels {
    void (*sym)(KArgs), (*terms)(KArgs), (*plain)(KArgs);
    int rows;          // anchor rows a workgroup owns
    int shares;        // shares of the J tiles its waves walk side by side
    size_t lds;        // dynamic LDS bytes
};

// The scalar outputs of a launch are [result | SGA_SLOTS slots] (loss_math.h).  A gs buffer carries ONE MORE block of (M+1)*8 doubles behind
// its slots, (2 + SGA_SLOTS) * (M+1)*8 doubles in all: the kernels read the float copy of 1/(sums+eps) from there (inv_sums_kernel writes it).
// The callers' allocations (loss_ops._aa_walk and the tests: slots + 1 blocks) follow this function.
static float* aa_inv_block(double* gs, int M) { return reinterpret_cast<float*>(gs + (size_t)(1 + SGA_SLOTS) * (M + 1) * 8); }

// Workgroups per row block: enough for `rounds` rounds of workgroups over the CUs, and no more than give every J share of a workgroup a
// tile (ntile column tiles of the kernel's own height, `shares` of them walked side by side).
static int aa_plan(int nib, int ntile, int shares, int rounds) {
    int nsp = (rounds * sga_num_cus() + nib - 1) / nib;
    if (nsp > (ntile + shares - 1) / shares) nsp = (ntile + shares - 1) / shares;
    return nsp < 1 ? 1 : nsp;
}

// The fields every A x A kernel reads, forward and backward (tables, split and outputs are the caller's).
static void aa_fill(AnchorMultiArgs& a, int M, const float* beta, int A, const double* sums, float alpha, float tau_icl, float tau_ial, int a_lo, int a_hi) {
    a.M = M; a.A = A; a.i_lo = a_lo; a.i_hi = a_hi; a.beta = beta; a.sums = sums; a.alpha = alpha;
    a.kc = LOG2E / tau_icl; a.ki = LOG2E / tau_ial; a.itc = 1.f / tau_icl; a.iti = 1.f / tau_ial;
}

static bool aa_symmetric(const AAContract& c, const AAOperands& o) {
    return c.walk == AA_SYMMETRIC || (c.walk == AA_EITHER && !(o.j_lo == 0 && o.j_hi == o.A && o.mir >= o.j_hi));
}

// Everything an entry point refuses, before anything is written or launched.
static int aa_validate(const AAContract& c, const AAOperands& o) {
    const int A = o.A, ra = c.row_align, ct = c.col_tile;
    SGA_CHECK_ARG(o.tables && o.beta && o.sums && o.coef && o.M1 && o.gs && o.gamma && A >= 0, "%s: bad argument", c.name);
    SGA_CHECK_ARG(o.M >= c.m_lo && o.M <= c.m_hi, "%s: M=%d not in %d..%d tables", c.name, o.M, c.m_lo, c.m_hi);
    SGA_CHECK_ARG(o.a_lo >= 0 && o.a_lo <= o.a_hi && o.a_hi <= A && o.a_lo % ra == 0 && (o.a_hi % ra == 0 || o.a_hi == A),
                  "%s: block [%d,%d) not on %d-row boundaries of [0,%d]", c.name, o.a_lo, o.a_hi, ra, A);
    SGA_CHECK_ARG(o.j_lo >= 0 && o.j_lo % ct == 0 && o.j_hi <= A && o.j_lo <= o.j_hi && (o.j_hi % ct == 0 || o.j_hi == A) && o.mir >= o.j_lo &&
                      (o.mir % ct == 0 || o.mir >= o.j_hi),
                  "%s: columns [%d,%d) / mirror start %d not on %d-column boundaries", c.name, o.j_lo, o.j_hi, o.mir, ct);
    if (aa_symmetric(c, o)) {
        // columns left of the mirror start are visited in the ordered way: they must lie in the block's own square
        SGA_CHECK_ARG(o.mir <= o.j_lo || (o.j_lo >= o.a_lo && (o.mir < o.j_hi ? o.mir : o.j_hi) <= o.a_hi),
                      "%s: ordered columns [%d,%d) outside the block's square [%d,%d)", c.name, o.j_lo, o.mir, o.a_lo, o.a_hi);
        SGA_CHECK_ARG(o.out_terms, "%s: a symmetric launch returns its terms (out_terms == NULL)", c.name);
    }
    for (int m = 0; m < o.M; ++m)      // (no mirrored elements, mir >= j_hi: no second stash)
        SGA_CHECK_ARG(o.tables[m] && o.M1[m] && (o.mir >= o.j_hi || (o.M2 && o.M2[m])), "%s: null table or stash", c.name);
    return SGA_OK;
}

// A validated job from the zeroing of its slots to the folds.  k: the kernel's argument struct with its table pointers set; a: the
// AnchorMultiArgs in it (k itself for the fp32 kernels).
template <class KArgs>
static int aa_run(const AAContract& c, const AAOperands& o, KArgs& k, AnchorMultiArgs& a, const AAKernels<KArgs>& kern, int threads, int rounds,
                  void* stream) {
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int M = o.M, NT = M + 1;
    if (int rc = zero_slots(o.gs, NT * 8, s, c.name)) return rc;
    if (int rc = zero_slots(o.gamma, M, s, c.name)) return rc;
    if (o.out_terms) { if (int rc = zero_slots(o.out_terms, NT + 2 * M, s, c.name)) return rc; }
    if (o.A == 0 || o.a_hi <= o.a_lo || o.j_hi <= o.j_lo) return SGA_OK;
    aa_fill(a, M, o.beta, o.A, o.sums, o.alpha, o.tau_icl, o.tau_ial, o.a_lo, o.a_hi);
    a.coef = o.coef; a.gs = o.gs; a.gamma = o.gamma; a.out = o.out_terms;
    a.j_lo = o.j_lo; a.j_hi = o.j_hi; a.mir = o.mir;
    for (int m = 0; m < M; ++m) { a.M1[m] = o.M1[m]; a.M2[m] = o.M2 ? o.M2[m] : nullptr; }
    float* inv = aa_inv_block(o.gs, M);
    hipLaunchKernelGGL(inv_sums_kernel, dim3(1), dim3(64), 0, s, o.sums, inv, NT * 8);
    a.inv = inv;
    // column tiles of 16: from j_lo to the end of the kernel's last column tile
    const int nib = (o.a_hi - o.a_lo + kern.rows - 1) / kern.rows, ntile16 = ((o.j_hi + c.col_tile - 1) / c.col_tile * c.col_tile - o.j_lo) / 16;
    a.nsplit = aa_plan(nib, ntile16, kern.shares, rounds);
    auto fn = aa_symmetric(c, o) ? kern.sym : o.out_terms ? kern.terms : kern.plain;
    hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kern.lds);
    hipLaunchKernelGGL(fn, dim3(nib * a.nsplit), dim3(threads), kern.lds, s, k);
    if (o.out_terms) fold_slots(o.out_terms, NT + 2 * M, s);
    fold_slots(o.gs, NT * 8, s);
    fold_slots(o.gamma, M, s);
    SGA_CHECK_LAUNCH(c.name);
    return SGA_OK;
}

}  // namespace
