// Internal: the owner / other row groups that every anchors x negatives sweep walks (the per-table kernels of loss_pertable.hip and the
// fused ones of contrastive.hip), and the plan that fills them for one packed table [X1 | X2 | N1 | N2].
#pragma once

struct SweepSeg { int row0, n, fam; };                 // other rows [row0, row0+n), sum family 0..3
struct SweepGroup { int own0, nown, blk0, nseg; SweepSeg seg[2]; int nsplit; };   // nsplit: multi kernel only

// Owner/other row groups of the sweeps.  [a_lo, a_hi) is the anchor shard this process owns (one process per GPU shards
// the anchors; 0..A on a single GPU): anchor-owner groups cover only the shard, negative-owner groups see only the shard's
// anchors as "others" -- summing the ranks' outputs gives the unsharded result.
// Fills grp[0..3] and returns the number of groups.
static inline int fill_groups(SweepGroup (&grp)[4], int A, int J1, int J2, bool grad, int a_lo, int a_hi) {
    const int x1 = 0, x2 = A, n1 = 2 * A, n2 = 2 * A + J1, ns = a_hi - a_lo;
    int blk = 0, g = 0;
    auto add = [&](int own0, int nown, SweepSeg s0, SweepSeg s1) {
        if (nown <= 0) return;
        SweepGroup& G = grp[g++];
        G.own0 = own0; G.nown = nown; G.blk0 = blk; G.nseg = 2; G.seg[0] = s0; G.seg[1] = s1; G.nsplit = 1;
        blk += (nown + 127) / 128;
    };
    add(x1 + a_lo, ns, SweepSeg{n1, J1, 0}, SweepSeg{n2, J2, 1});       // s11, s12
    add(x2 + a_lo, ns, SweepSeg{n2, J2, 2}, SweepSeg{n1, J1, 3});       // s22, s21
    if (grad) {
        add(n1, J1, SweepSeg{x1 + a_lo, ns, 0}, SweepSeg{x2 + a_lo, ns, 3});
        add(n2, J2, SweepSeg{x1 + a_lo, ns, 1}, SweepSeg{x2 + a_lo, ns, 2});
    }
    return g;
}
