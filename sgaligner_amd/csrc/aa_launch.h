// The host side of the anchors x anchors backward, once for every kernel that ends in aa_epilogue.h (loss_anchor.hip: fp32 MFMA over the
// packed tables; anchor3.hip: bf16 MFMA over the three-plane image): what an entry point accepts (AAContract), the checks of a job against
// it (aa_validate), the split plan (aa_plan) and everything from the zeroing of the slots to the folds (aa_run).  An entry point is its
// contract, its kernels (AAKernels) with their LDS size and grid numbers, the table pointers in its kernel's own argument struct, one call.
#pragma once
#include <algorithm>
#include <mutex>

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
struct AAGeom {
    int rows;          // anchor rows a workgroup owns
    int shares;        // shares of the J tiles its waves walk side by side
    int col_tile;      // the kernel's column tile (the contract's)
    int rounds;        // whole rounds of workgroups the first run of the plan has at least (aa_plan)
};

template <class KArgs>
struct AAKernels {
    void (*sym)(KArgs), (*terms)(KArgs), (*plain)(KArgs);
    AAGeom g;
    size_t lds;        // dynamic LDS bytes
};

// The scalar outputs of a launch are [result | SGA_SLOTS slots] (loss_math.h).  A gs buffer carries ONE MORE block of (M+1)*8 doubles behind
// its slots, (2 + SGA_SLOTS) * (M+1)*8 doubles in all: the kernels read the float copy of 1/(sums+eps) from there (inv_sums_kernel writes it).
// The callers' allocations (loss_ops._aa_walk and the tests: slots + 1 blocks) follow this function.
static float* aa_inv_block(double* gs, int M) { return reinterpret_cast<float*>(gs + (size_t)(1 + SGA_SLOTS) * (M + 1) * 8); }

// The numbers of the two kernel families, in one place for the entry points and for the plan query (sga_loss_anchor_plan): the three-plane
// kernels (anchor3.hip) and the fp32 ones (loss_anchor.hip: 32 rows and two J shares up to three tables, 16 rows and four shares for four).
// rounds, timed (profiles/aa_fill_bench_aa.txt): three-plane, the 19 launches of the configs[2] walk, 413.6 / 413.1 / 414.2 ms with 1 / 2 / 3 --
// no difference, so the fewest workgroups; fp32, the symmetric 2048 x 155 648 block, 13.09 ms with 2 and 12.52 with 3 (what it had: 12.4 .. 12.6).
constexpr AAGeom aa_geom(bool planes, int M) { return planes ? AAGeom{32, 4, 32, 1} : M <= 3 ? AAGeom{32, 2, 16, 3} : AAGeom{16, 4, 16, 3}; }

// The launch plan.  A workgroup is (row block, split s of n): it walks the steps s, s + n, s + 2n, ... of its row block, a step being
// `shares` column tiles side by side.  With one n for the whole job (the plan up to now: n = ceil(rounds * CUs / nib)) the workgroups are
// equal, nib * n of them run in ceil(nib * n / slots) rounds and the last round is part-filled: 0.85 of the slots busy over the walk of
// configs[2], 0.755 in its worst launch.  Now the job is two runs of row blocks.  The first nib1 row blocks are cut n1 ways so
// that they fill F whole rounds (nib1 * n1 <= F * slots, fewer than n1 slots short); the nib - nib1 row blocks left over, less than a
// round of work, are cut n2 ways, usually much finer, so that they fill the last round too.  Long workgroups first, short ones behind them
// is also the order that lets the dispatcher level what the model does not know (a slow CU, a ragged last tile).
//
// Why not equal contiguous ranges of (row block, step), cut without regard to the row blocks, one per workgroup: built and measured on
// the three-plane kernels (256 equal-cost ranges, a prologue per row block a range touches, consecutive steps), the walk of configs[2]
// took 497.6 ms against 425.6 ms for this plan on the same machine, as slow as the part-filled rounds it was to cure
// (profiles/aa_fill_contiguous_ranges.txt).  The reading, by arithmetic only: under the interleaved walk the workgroups resident together
// share a split index over 256 / n row blocks and read the same J fragments at about the same time (240 KiB per step and workgroup at
// M = 3, 3 to 4 TB/s over the chip, from an image of 600 MB at configs[2]), n streams that L2 serves; ranges that start at 256 different
// steps are 256 streams.  Of the two ways to give every workgroup of a row block the same cost, this is the interleaving, not the
// weighting: every split of a row block of a symmetric job gets the same mix of own-square tiles (ordered epilogue; 0.72 of a mirrored
// step's time, same file) and mirrored ones to within one step, so equal step counts are equal cost.  The kernels keep their loop; they
// decode (row block, split, n) from three integers (aa_epilogue.h: aa_unit).  Measured on the configs[2] walk: 495.3 -> 413.6 ms.
//
// Model: a workgroup with n splits costs ceil(steps / n) + 1 steps (the 1: its prologue and last flush), rounds are synchronous.  The
// search takes the (n1, n2) with the shortest modelled time, then the fewest workgroups.
struct AAPlan { int nib1, n1, n2, wgs; long long cost; };

static AAPlan aa_plan(int nib, int ntile, int shares, int slots, int rounds, bool two_runs = true) {
    const int steps = (ntile + shares - 1) / shares, cap = steps < 1 ? 1 : steps;
    if (slots < 1) slots = 1;
    if (nib < 1) return {0, 1, 1, 0, 0};
    auto cdiv = [](long long a, long long b) { return (a + b - 1) / b; };
    const int want = (int)cdiv((long long)rounds * slots, nib);                 // the fewest splits with `rounds` whole rounds
    const int lo1 = std::min(want, cap), hi1 = std::min(lo1 + 15, cap), hi2 = two_runs ? std::min(cap, std::max(hi1, 64)) : 0;
    AAPlan best = {0, 1, 1, 0, -1};
    auto take = [&](int nib1, int n1, int n2, long long cost) {
        const int wgs = nib1 * n1 + (nib - nib1) * n2;
        if (best.cost < 0 || cost < best.cost || (cost == best.cost && wgs < best.wgs)) best = {nib1, n1, n2, wgs, cost};
    };
    for (int n1 = lo1; n1 <= hi1; ++n1) {
        const long long c1 = cdiv(steps, n1) + 1;
        take(nib, n1, n1, cdiv((long long)nib * n1, slots) * c1);                // one run
        const long long F = (long long)nib * n1 / slots;
        const int nib1 = (int)(F * slots / n1);
        if (nib1 >= nib) continue;
        for (int n2 = 1; n2 <= hi2; ++n2) take(nib1, n1, n2, F * c1 + cdiv((long long)(nib - nib1) * n2, slots) * (cdiv(steps, n2) + 1));
    }
    return best;
}

// The plan of a backward job: its row blocks, and its column tiles of 16 from j_lo to the end of the kernel's last column tile.
static AAPlan aa_job_plan(const AAGeom& g, int a_lo, int a_hi, int j_lo, int j_hi, int slots) {
    const int nib = (a_hi - a_lo + g.rows - 1) / g.rows, ntile16 = ((j_hi + g.col_tile - 1) / g.col_tile * g.col_tile - j_lo) / 16;
    return aa_plan(nib, ntile16, g.shares, slots, g.rounds);
}

// Workgroups of `fn` a CU holds at once with this launch's dynamic LDS, times the CUs: the slots of the plan.  Asked once per kernel and
// device.  The table is per translation unit (12 kernels in loss_anchor.hip, 6 in anchor3.hip, one process per GPU: sgaligner_amd/dist.py);
// an entry that does not fit is asked again at every launch, which costs time and nothing else.
static int aa_slots(const void* fn, int threads, size_t lds) {
    struct Seen { const void* fn; int dev, per_cu; };
    constexpr int NSEEN = 32;
    static Seen seen[NSEEN];
    static int nseen = 0;
    static std::mutex mu;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) { (void)hipGetLastError(); dev = 0; }
    std::lock_guard<std::mutex> lock(mu);
    for (int i = 0; i < nseen; ++i)
        if (seen[i].fn == fn && seen[i].dev == dev) return seen[i].per_cu * sga_num_cus();
    int per_cu = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, threads, lds) != hipSuccess || per_cu < 1) { (void)hipGetLastError(); per_cu = 1; }
    if (nseen < NSEEN) seen[nseen++] = {fn, dev, per_cu};
    return per_cu * sga_num_cus();
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
static int aa_run(const AAContract& c, const AAOperands& o, KArgs& k, AnchorMultiArgs& a, const AAKernels<KArgs>& kern, int threads, void* stream) {
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
    auto fn = aa_symmetric(c, o) ? kern.sym : o.out_terms ? kern.terms : kern.plain;
    hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kern.lds);
    const AAPlan p = aa_job_plan(kern.g, o.a_lo, o.a_hi, o.j_lo, o.j_hi, aa_slots(reinterpret_cast<const void*>(fn), threads, kern.lds));
    a.nib1 = p.nib1; a.nsplit = p.n1; a.nsplit2 = p.n2;
    hipLaunchKernelGGL(fn, dim3(p.wgs), dim3(threads), kern.lds, s, k);
    if (o.out_terms) fold_slots(o.out_terms, NT + 2 * M, s);
    fold_slots(o.gs, NT * 8, s);
    fold_slots(o.gamma, M, s);
    SGA_CHECK_LAUNCH(c.name);
    return SGA_OK;
}

}  // namespace
