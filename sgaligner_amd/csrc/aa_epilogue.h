// What the anchors x anchors backward kernels share once a lane holds its similarities (loss_anchor.hip: fp32 MFMA over the packed tables;
// anchor3.hip: bf16 MFMA over the three-plane image): the launch arguments, the per-element epilogue in its ordered and symmetric forms and
// the hand-over of the fp32 partial sums to the fp64 slots.  Their host side is aa_launch.h.  A lane holds P[m][r] = S_m[i, j], Q[m][r] = S_m[j, i] for its anchor row
// i = my_i and the four columns j = jg + r; which (lane, r) maps to which column is the calling kernel's business (jg).
#pragma once
#include "loss_math.h"

namespace {

struct AnchorMultiArgs {
    int M, A, i_lo, i_hi, nsplit;
    const float* Z[4];
    const float* beta;             // [M]
    const double* sums;            // [(M+1)][8]
    const float* inv;              // [(M+1)][8] = 1/(sums + 1e-9) as floats (inv_sums_kernel): uniform global loads -> SGPRs
    float alpha, kc, ki, itc, iti;
    double* out;                   // fwd: [(M+1) + 2M] (+ slots)
    const float* coef;             // bwd: dL/d(out)
    float* M1[4];                  // bwd: M1[m][j*ns + (i - i_lo)] = dL/dS_m[i,j] (+ beta_m dL/dS_J)
    double* gs;                    // bwd: [(M+1)][8] (+ slots)
    double* gamma;                 // bwd: [M] (+ slots)
    int j_lo;                      // bwd: first column (a multiple of 16); stash rows are j - j_lo.  0 except in the symmetric mode
    float* M2[4];                  // symmetric mode: M2[m][(j - mir)*ns + (i - i_lo)] = the MIRRORED coefficient dL/dS_m[j,i], j >= mir
    int j_hi, mir;                 // symmetric mode: columns [j_lo, j_hi); tiles at j >= mir also produce the mirrored element (one GPU: A, i_hi)
    int nib1, nsplit2;             // bwd: row blocks [0, nib1) are cut into nsplit workgroups each, the row blocks behind them into nsplit2 (aa_plan)
};

// Workgroup -> (row block ib, share `split` of `ns` of its J tiles): the launch plan of aa_launch.h, two runs of row blocks with a split
// count each.  Workgroup-uniform: scalar registers only.
__device__ __forceinline__ void aa_unit(const AnchorMultiArgs& a, int& ib, int& split, int& ns) {
    const int b = blockIdx.x, n1 = a.nib1 * a.nsplit;
    if (b < n1) { ns = a.nsplit; ib = b / ns; split = b - ib * ns; }
    else { ns = a.nsplit2; ib = (b - n1) / ns; split = (b - n1) - ib * ns; ib += a.nib1; }
}

__global__ void inv_sums_kernel(const double* __restrict__ sums, float* __restrict__ inv, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) inv[i] = (float)(1.0 / (sums[i] + 1e-9));
}

// All running sums are fp32 per lane and leave for the fp64 slots every 32 tiles (<= 128 addends per partial): at configs[2] a lane
// sees thousands of nearly equal addends, whose fp32 rounding is a bias, not a random walk (1.7e-4 on the IAL terms with
// whole-sweep fp32 partials; tools/dbg/aa_check64.py).
template <int M, bool TERMS>
__device__ __forceinline__ void aa_flush(const AnchorMultiArgs& a, const float* inv_s, const int lane, const int slot,
                                         float (&acc_gs)[M + 1][8], float (&acc_gam)[M], float (&acc_out)[TERMS ? 3 * M + 1 : 1]) {
    constexpr int NT = M + 1;
    if (TERMS) {
#pragma unroll
        for (int e = 0; e < NT + 2 * M; ++e) {
            const float v = wave_sum(acc_out[TERMS ? e : 0]);
            if (lane == 0 && v != 0.f) atomicAdd(a.out + (NT + 2 * M) * (1 + slot) + e, (double)v);
            acc_out[TERMS ? e : 0] = 0.f;
        }
    }
#pragma unroll
    for (int k = 0; k < NT; ++k)
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float iv2 = inv_s[k * 8 + e];
            const float v = -iv2 * iv2 * wave_sum(acc_gs[k][e]);          // dg/dsum = -d inv^2 (g/u)^2: the uniform factor, once
            if (lane == 0 && v != 0.f) atomicAdd(a.gs + NT * 8 * (1 + slot) + k * 8 + e, (double)v);
            acc_gs[k][e] = 0.f;
        }
#pragma unroll
    for (int m = 0; m < M; ++m) {
        const float v = wave_sum(acc_gam[m]);
        if (lane == 0 && v != 0.f) atomicAdd(a.gamma + M * (1 + slot) + m, (double)v);
        acc_gam[m] = 0.f;
    }
}

// One element (r) at a time, with a scheduling barrier between elements: interleaving the four independent chains keeps ~4x the
// temporaries live and pushes the loop into scratch.  Masks are multiplied in (rows/columns past the end are finite -- clamped copies of
// valid rows, or the image's zero padding rows -- so every intermediate is finite): selects here become 28 exec-mask branches.
// MASKED = false: interior tiles (all anchor rows and all columns valid) -- the ~20 multiplications by okf and the predicated stores are
// 4 % of this VALU-bound loop.
template <int M, bool TERMS, bool MASKED>
__device__ __forceinline__ void aa_epilogue(const AnchorMultiArgs& a, const float* inv_s, const float (&beta)[M], const f32x4 (&P)[M],
                                            const f32x4 (&Q)[M], float (&acc_gs)[M + 1][8], float (&acc_gam)[M], float (&acc_out)[TERMS ? 3 * M + 1 : 1],
                                            const int jg, const int JH, const bool iv, const int my_i, const int ns) {
    constexpr int NT = M + 1;
    auto CF = [&](int e) { return a.coef[e]; };
    const float* js = inv_s + M * 8;
    const float cJ = CF(M);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int j = jg + r;
        const bool ok = !MASKED || (iv && (j < JH));
        const float okf = (!MASKED || ok) ? 1.f : 0.f;
        float xj = 0.f, yj = 0.f;
#pragma unroll
        for (int m = 0; m < M; ++m) { xj = fmaf(beta[m], P[m][r], xj); yj = fmaf(beta[m], Q[m][r], yj); }
        float gJ, EA = 0.f, EB = 0.f;
        // joint ICL
        {
            const float dx = fexp2(xj * a.kc), dy = fexp2(yj * a.kc);
            const GP Ax = g_parts(dx, js[0], js[2]), Bx = g_parts(dx, js[4], js[6]);
            const float qAy = g_val(dy, js[0], js[2]), qBy = g_val(dy, js[4], js[6]);
            const float denA = a.alpha * Ax.q + (1.f - a.alpha) * qBy;
            const float wA = okf * (-cJ * a.alpha) * frcp(denA) * dx;      // weight * d
            const float wB = okf * (-cJ * (1.f - a.alpha)) * frcp(a.alpha * qAy + (1.f - a.alpha) * Bx.q) * dx;
            if (TERMS) acc_out[TERMS ? M : 0] = fmaf(okf, -flog(denA), acc_out[TERMS ? M : 0]);     // -log(a qA(x) + (1-a) qB(y)), losses.py:55-57
            gJ = fmaf(wA, Ax.dd, wB * Bx.dd) * a.itc;
            acc_gs[M][0] = fmaf(wA, Ax.p, acc_gs[M][0]); acc_gs[M][2] = fmaf(wA, Ax.r, acc_gs[M][2]);
            acc_gs[M][4] = fmaf(wB, Bx.p, acc_gs[M][4]); acc_gs[M][6] = fmaf(wB, Bx.r, acc_gs[M][6]);
        }
        // joint IAL reference distribution (qm), shared by every modality
        const float dji = fexp2(xj * a.ki);
        const GP MA = g_parts(dji, js[1], js[3]), MB = g_parts(dji, js[5], js[7]);
        const float lqma = flog(MA.q), lqmb = flog(MB.q);
        float gx[M];
        // per modality ICL + IAL (qo part)
#pragma unroll
        for (int m = 0; m < M; ++m) {
            const float* is = inv_s + m * 8;
            const float c = CF(m), ca = CF(NT + m), cb = CF(NT + M + m);
            const float x = P[m][r], y = Q[m][r];
            const float dx = fexp2(x * a.kc), dy = fexp2(y * a.kc);
            const GP Ax = g_parts(dx, is[0], is[2]), Bx = g_parts(dx, is[4], is[6]);
            const float qAy = g_val(dy, is[0], is[2]), qBy = g_val(dy, is[4], is[6]);
            const float denA = a.alpha * Ax.q + (1.f - a.alpha) * qBy;
            const float wA = okf * (-c * a.alpha) * frcp(denA) * dx;
            const float wB = okf * (-c * (1.f - a.alpha)) * frcp(a.alpha * qAy + (1.f - a.alpha) * Bx.q) * dx;
            if (TERMS) acc_out[TERMS ? m : 0] = fmaf(okf, -flog(denA), acc_out[TERMS ? m : 0]);
            float gxm = fmaf(wA, Ax.dd, wB * Bx.dd) * a.itc;
            acc_gs[m][0] = fmaf(wA, Ax.p, acc_gs[m][0]); acc_gs[m][2] = fmaf(wA, Ax.r, acc_gs[m][2]);
            acc_gs[m][4] = fmaf(wB, Bx.p, acc_gs[m][4]); acc_gs[m][6] = fmaf(wB, Bx.r, acc_gs[m][6]);
            const float dm = fexp2(x * a.ki);
            const GP OA = g_parts(dm, is[1], is[3]), OB = g_parts(dm, is[5], is[7]);
            const float xA = okf * __expf(OA.q), xB = okf * __expf(OB.q);
            const float eA = ca * xA, eB = cb * xB;
            if (TERMS) {                                                       // exp(qo) (qo - log qm): KLDiv with log_target, losses.py:90-94
                acc_out[TERMS ? NT + m : 0] = fmaf(xA, OA.q - lqma, acc_out[TERMS ? NT + m : 0]);
                acc_out[TERMS ? NT + M + m : 0] = fmaf(xB, OB.q - lqmb, acc_out[TERMS ? NT + M + m : 0]);
            }
            const float tA = eA * (OA.q - lqma + 1.f) * dm, tB = eB * (OB.q - lqmb + 1.f) * dm;
            gxm = fmaf(fmaf(tA, OA.dd, tB * OB.dd), a.iti, gxm);
            acc_gs[m][1] = fmaf(tA, OA.p, acc_gs[m][1]); acc_gs[m][3] = fmaf(tA, OA.r, acc_gs[m][3]);
            acc_gs[m][5] = fmaf(tB, OB.p, acc_gs[m][5]); acc_gs[m][7] = fmaf(tB, OB.r, acc_gs[m][7]);
            EA += eA; EB += eB;
            gx[m] = gxm;
        }
        // joint IAL (qm part), totals + stash
        {
            const float uA = -EA * frcp(MA.q) * dji, uB = -EB * frcp(MB.q) * dji;
            gJ = fmaf(fmaf(uA, MA.dd, uB * MB.dd), a.iti, gJ);
            acc_gs[M][1] = fmaf(uA, MA.p, acc_gs[M][1]); acc_gs[M][3] = fmaf(uA, MA.r, acc_gs[M][3]);
            acc_gs[M][5] = fmaf(uB, MB.p, acc_gs[M][5]); acc_gs[M][7] = fmaf(uB, MB.r, acc_gs[M][7]);
        }
#pragma unroll
        for (int m = 0; m < M; ++m) {
            acc_gam[m] = fmaf(gJ, P[m][r], acc_gam[m]);
            if (ok) a.M1[m][(size_t)(j - a.j_lo) * ns + (my_i - a.i_lo)] = fmaf(beta[m], gJ, gx[m]);
        }
        // pin the running sums here: otherwise their updates are sunk into the loop latch (they are only
        // consumed by the next iteration) and every factor of all four elements stays live until then
#pragma unroll
        for (int k = 0; k < NT; ++k)
#pragma unroll
            for (int e = 0; e < 8; ++e) asm volatile("" : "+v"(acc_gs[k][e]));
#pragma unroll
        for (int m = 0; m < M; ++m) asm volatile("" : "+v"(acc_gam[m]));
        if (TERMS) {
#pragma unroll
            for (int e = 0; e < NT + 2 * M; ++e) asm volatile("" : "+v"(acc_out[TERMS ? e : 0]));
        }
        __builtin_amdgcn_sched_barrier(0);
    }
}

// Symmetric epilogue: elements (i, j) [x = P, "dir 0", stash M1] and (j, i) [y = Q, "dir 1", stash M2] together.
template <int M>
__device__ __forceinline__ void aa_epilogue_sym(const AnchorMultiArgs& a, const float* inv_s, const float (&beta)[M], const f32x4 (&P)[M],
                                                const f32x4 (&Q)[M], float (&acc_gs)[M + 1][8], float (&acc_gam)[M], float (&acc_out)[3 * M + 1],
                                                const int jg, const int JH, const bool iv, const int my_i, const int ns) {
    constexpr int NT = M + 1;
    constexpr bool TERMS = true;
    auto CF = [&](int e) { return a.coef[e]; };
    const float* js = inv_s + M * 8;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int j = jg + r;
        const bool ok = iv && (j < JH);
        const float okf = ok ? 1.f : 0.f;
        float xj = 0.f, yj = 0.f;
#pragma unroll
        for (int m = 0; m < M; ++m) { xj = fmaf(beta[m], P[m][r], xj); yj = fmaf(beta[m], Q[m][r], yj); }
        float gci[NT][2];                                        // ICL part of dL/dx, dL/dy per table (joint = M)
        // ---- ICL, every table and the joint: term(i,j) = -log(a qA(x) + (1-a) qB(y)), term(j,i) = -log(a qA(y) + (1-a) qB(x))
#pragma unroll
        for (int k = 0; k < NT; ++k) {
            const float* is = inv_s + k * 8;
            const float x = k < M ? P[k < M ? k : 0][r] : xj, y = k < M ? Q[k < M ? k : 0][r] : yj;
            const float c = CF(k);
            const float dx = fexp2(x * a.kc), dy = fexp2(y * a.kc);
            const GP Ax = g_parts(dx, is[0], is[2]), Bx = g_parts(dx, is[4], is[6]);
            const GP Ay = g_parts(dy, is[0], is[2]), By = g_parts(dy, is[4], is[6]);
            const float den1 = a.alpha * Ax.q + (1.f - a.alpha) * By.q;
            const float den2 = a.alpha * Ay.q + (1.f - a.alpha) * Bx.q;
            const float r1 = okf * -c * frcp(den1), r2 = okf * -c * frcp(den2);
            const float wAx = a.alpha * r1 * dx, wBx = (1.f - a.alpha) * r2 * dx;
            const float wAy = a.alpha * r2 * dy, wBy = (1.f - a.alpha) * r1 * dy;
            acc_out[TERMS ? k : 0] = fmaf(okf, -(flog(den1) + flog(den2)), acc_out[TERMS ? k : 0]);
            gci[k][0] = fmaf(wAx, Ax.dd, wBx * Bx.dd) * a.itc;
            gci[k][1] = fmaf(wAy, Ay.dd, wBy * By.dd) * a.itc;
            acc_gs[k][0] = fmaf(wAx, Ax.p, fmaf(wAy, Ay.p, acc_gs[k][0])); acc_gs[k][2] = fmaf(wAx, Ax.r, fmaf(wAy, Ay.r, acc_gs[k][2]));
            acc_gs[k][4] = fmaf(wBx, Bx.p, fmaf(wBy, By.p, acc_gs[k][4])); acc_gs[k][6] = fmaf(wBx, Bx.r, fmaf(wBy, By.r, acc_gs[k][6]));
#pragma unroll
            for (int e = 0; e < 8; e += 2) asm volatile("" : "+v"(acc_gs[k][e]));
            asm volatile("" : "+v"(acc_out[TERMS ? k : 0]));
            __builtin_amdgcn_sched_barrier(0);
        }
        // ---- IAL, one direction at a time (nothing shared between x and y here)
#pragma unroll
        for (int dir = 0; dir < 2; ++dir) {
            const float vj = dir ? yj : xj;
            const float dji = fexp2(vj * a.ki);
            const GP MA = g_parts(dji, js[1], js[3]), MB = g_parts(dji, js[5], js[7]);
            const float lqma = flog(MA.q), lqmb = flog(MB.q);
            float gx[M], EA = 0.f, EB = 0.f;
#pragma unroll
            for (int m = 0; m < M; ++m) {
                const float* is = inv_s + m * 8;
                const float ca = CF(NT + m), cb = CF(NT + M + m);
                const float v = dir ? Q[m][r] : P[m][r];
                const float dm = fexp2(v * a.ki);
                const GP OA = g_parts(dm, is[1], is[3]), OB = g_parts(dm, is[5], is[7]);
                const float xA = okf * __expf(OA.q), xB = okf * __expf(OB.q);
                const float eA = ca * xA, eB = cb * xB;
                acc_out[TERMS ? NT + m : 0] = fmaf(xA, OA.q - lqma, acc_out[TERMS ? NT + m : 0]);
                acc_out[TERMS ? NT + M + m : 0] = fmaf(xB, OB.q - lqmb, acc_out[TERMS ? NT + M + m : 0]);
                const float tA = eA * (OA.q - lqma + 1.f) * dm, tB = eB * (OB.q - lqmb + 1.f) * dm;
                gx[m] = fmaf(fmaf(tA, OA.dd, tB * OB.dd), a.iti, gci[m][dir]);
                acc_gs[m][1] = fmaf(tA, OA.p, acc_gs[m][1]); acc_gs[m][3] = fmaf(tA, OA.r, acc_gs[m][3]);
                acc_gs[m][5] = fmaf(tB, OB.p, acc_gs[m][5]); acc_gs[m][7] = fmaf(tB, OB.r, acc_gs[m][7]);
                EA += eA; EB += eB;
            }
            const float uA = -EA * frcp(MA.q) * dji, uB = -EB * frcp(MB.q) * dji;
            const float gJ = fmaf(fmaf(uA, MA.dd, uB * MB.dd), a.iti, gci[M][dir]);
            acc_gs[M][1] = fmaf(uA, MA.p, acc_gs[M][1]); acc_gs[M][3] = fmaf(uA, MA.r, acc_gs[M][3]);
            acc_gs[M][5] = fmaf(uB, MB.p, acc_gs[M][5]); acc_gs[M][7] = fmaf(uB, MB.r, acc_gs[M][7]);
            float* const* dst = dir ? a.M2 : a.M1;
            const size_t off = (size_t)(j - (dir ? a.mir : a.j_lo)) * ns + (my_i - a.i_lo);
#pragma unroll
            for (int m = 0; m < M; ++m) {
                acc_gam[m] = fmaf(gJ, dir ? Q[m][r] : P[m][r], acc_gam[m]);
                if (ok) dst[m][off] = fmaf(beta[m], gJ, gx[m]);
            }
#pragma unroll
            for (int k = 0; k < NT; ++k)
#pragma unroll
                for (int e = 1; e < 8; e += 2) asm volatile("" : "+v"(acc_gs[k][e]));
#pragma unroll
            for (int m = 0; m < M; ++m) asm volatile("" : "+v"(acc_gam[m]));
#pragma unroll
            for (int e = NT; e < NT + 2 * M; ++e) asm volatile("" : "+v"(acc_out[TERMS ? e : 0]));
            __builtin_amdgcn_sched_barrier(0);
        }
    }
}

}  // namespace
