"""NumPy restatement of the sparse GAT route's graph structure (sgaligner_amd/csrc/gat_sparse.hip; no tests in this module).

Rules (those of the dense kernels' prologue and of oracle.sga_oracle._canon_edges): input self loops and endpoints outside [0, N_g) are
dropped, every node gets exactly one self loop, duplicate pairs keep their multiplicity.  Node ids are batch-global.
    row_ptr [T+1], src [U], mult [U]     target-major, the sources of a target ascending
    col_ptr [T+1], tgt [U], perm [U]     the transpose: sources ascending, the targets of a source ascending; perm indexes the target-major entry"""
import numpy as np


def csr(graphs):
    """graphs: (nodes, edges [E, 2] int64 graph-local (source, target), ...) per graph -> dict of int64 arrays and U."""
    ii, jj, n0 = [], [], 0
    for g in graphs:
        n, e = int(g[0]), np.asarray(g[1], dtype=np.int64).reshape(-1, 2)
        s, d = e[:, 0], e[:, 1]
        ok = (s != d) & (s >= 0) & (s < n) & (d >= 0) & (d < n)
        ii += [d[ok] + n0, np.arange(n0, n0 + n)]
        jj += [s[ok] + n0, np.arange(n0, n0 + n)]
        n0 += n
    T = n0
    ii = np.concatenate(ii + [np.zeros(0, dtype=np.int64)]).astype(np.int64)
    jj = np.concatenate(jj + [np.zeros(0, dtype=np.int64)]).astype(np.int64)
    keys, mult = np.unique(ii * (1 << 32) + jj, return_counts=True)          # ascending (target, source)
    ti, sj = keys >> 32, keys & 0xffffffff
    row_ptr = np.concatenate([[0], np.cumsum(np.bincount(ti, minlength=T))]).astype(np.int64)
    perm = np.lexsort((ti, sj))                                              # by source, then target
    col_ptr = np.concatenate([[0], np.cumsum(np.bincount(sj, minlength=T))]).astype(np.int64)
    return dict(T=T, U=int(keys.shape[0]), row_ptr=row_ptr, src=sj, mult=mult.astype(np.int64), col_ptr=col_ptr, tgt=ti[perm], perm=perm)


def expand(c):
    """The (source, target) multiset of a structure, expanded by multiplicity and sorted: [sum mult, 2]."""
    tgt = np.repeat(np.arange(c['T']), np.diff(c['row_ptr']))
    pairs = np.stack([np.repeat(c['src'], c['mult']), np.repeat(tgt, c['mult'])], 1)
    return pairs[np.lexsort((pairs[:, 0], pairs[:, 1]))]
