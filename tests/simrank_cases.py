"""Tie-dense embeddings on which every similarity route of csrc/simrank.hip is EXACT, and a plain fp64 reference of what the
kernels decide from them (test helper; importable without a GPU).

A row has exactly `nnz` (4 / 16 / 64 / 256) non-zero entries, each +-1, times one power of two in [1/4, 4].  Its norm is
sqrt(nnz) 2^s, a power of two, so every normalised entry is +-2^-k (representable in fp16) and every dot product of two
normalised rows is an integer over nnz: fp64, the fp32 MFMA routes and both fp16 routes compute the SAME numbers whatever
the order of accumulation, and equal distances are true ties.  Rank, top-K, Hits@K, SGAR and the node correspondences are
then integers that every route has to reproduce without a tolerance -- and the stable tie-break (lower object index
first) decides a good part of them.

Pairs are laid out like synthetic.make_batch: `ns` source objects, then the reference objects; anchor i of a pair is the
source object i, its target the reference object ns + i.  ns is even wherever a pair has anchors, so a target has the parity
of its anchor."""
import numpy as np

NNZ_CHOICES = (4, 16, 64, 256)


def nnz_for(D):
    """The largest row weight of NNZ_CHOICES that fits D columns."""
    return max(z for z in NNZ_CHOICES if z <= D)


def split_of(n):
    """(ns, anchors) of an n-object pair: an even number of source objects, about 2/3 of them anchors; pairs of fewer than 4
    objects have no anchors."""
    if n < 4:
        return n // 2, 0
    ns = 2 * (n // 4)
    return ns, max(1, (2 * ns) // 3)


def _fresh_row(rng, D, nnz, local_idx):
    """nnz entries of +-1 on a random support that holds the columns D-1 and D-2 for an even row, column 0 for an odd one: the
    scalar tail of a K group / the zero-filled padding's neighbours and the first group always carry weight."""
    forced = [D - 1, D - 2] if local_idx % 2 == 0 else [0]
    rest = np.setdiff1d(np.arange(D), forced)
    sup = np.concatenate([forced, rng.choice(rest, nnz - len(forced), replace=False)]).astype(np.int64)
    row = np.zeros(D)
    row[sup] = rng.choice([-1.0, 1.0], nnz)
    return row


def _flipped(rng, row, nnz, f=None):
    """`row` with f of its signs flipped, f drawn from [nnz/4, nnz/2]: the dot with the original is (nnz - 2f)/nnz in [0, 1/2]."""
    f = int(rng.integers(nnz // 4, nnz // 2 + 1)) if f is None else f
    sup = np.flatnonzero(row)
    out = row.copy()
    out[rng.choice(sup, f, replace=False)] *= -1.0
    return out


def make_case(D, pair_sizes, seed, nnz=None, anchors=None, lone_anchor_pair=None, equal_f=()):
    """One batch.  anchors: per-pair anchor counts (default split_of); equal_f: pairs whose anchors all get the same f;
    lone_anchor_pair: index of a 1-object pair that gets one
    anchor whose target is the LAST object of the pair before it (outside the pair: no rank, a miss).
    Returns dict(emb [T,D] fp64, D, nnz, counts, offs, ns, na, data_dict)."""
    nnz = nnz_for(D) if nnz is None else nnz
    assert nnz <= D and D >= 3
    rng = np.random.default_rng(seed)
    counts = np.asarray(pair_sizes, dtype=np.int64)
    offs = np.concatenate([[0], np.cumsum(counts)])
    rows, ns_all, na_all, e1i, e2i = [], [], [], [], []
    for b, n in enumerate(counts):
        n = int(n)
        ns, a = split_of(n)
        if anchors is not None:
            a = int(anchors[b])
            assert a == 0 or (ns % 2 == 0 and a <= min(ns, n - ns))
        E = np.stack([_fresh_row(rng, D, nnz, i) for i in range(n)])
        same = lambda lo, hi, par: [j for j in range(lo, hi) if j % 2 == par]
        # a two-anchor pair of `equal_f`: both matches are equally far, and with the duplicates below one of the two predictions
        # is right and one wrong at the SAME top-1 distance -- SGAR '50' then hangs on the stable order of the anchors alone
        f2 = int(rng.integers(nnz // 4, nnz // 2 + 1)) if b in equal_f else None
        if a:
            E[ns] = _flipped(rng, E[0], nnz, f2)
        # a query identical to another query's target (pairs of 8 anchors or more): an anchor of the parity of anchor 0's target
        # becomes a copy of that target, and is at distance 0 from it
        if a >= 8:
            E[same(1, a, ns % 2)[-1]] = E[ns]
        for i in range(1, a):
            E[ns + i] = _flipped(rng, E[i], nnz, f2)
        # exact duplicates of a target BELOW it (anchor 1's target, copied to a source object that is no anchor) and of another
        # target ABOVE it (the last anchor's target -- anchor 0's where there are two --, copied to a reference object that is no
        # target), each at an index of the target's parity: which of the two equal distances wins is the tie-break alone
        if a >= 2:
            t_hi = ns + a - 1 if a >= 3 else ns
            lo, hi = same(a, ns, (ns + 1) % 2), same(ns + a, n, t_hi % 2)
            if lo:
                E[lo[0]] = E[ns + 1]
            if hi:
                E[hi[-1]] = E[t_hi]
        E *= 2.0 ** rng.integers(-2, 3, size=(n, 1))
        rows.append(E)
        ns_all.append(ns)
        if lone_anchor_pair is not None and b == lone_anchor_pair:
            assert n == 1 and b > 0 and a == 0
            e1i.append(int(offs[b]))
            e2i.append(int(offs[b]) - 1)
            a = 1
        else:
            e1i += [int(offs[b]) + i for i in range(a)]
            e2i += [int(offs[b]) + ns + i for i in range(a)]
        na_all.append(a)
    ns_all, na_all = np.asarray(ns_all, dtype=np.int64), np.asarray(na_all, dtype=np.int64)
    dd = {'batch_size': len(counts), 'tot_obj_count': counts.copy(), 'e1i_count': na_all.copy(),
          'e1i': np.asarray(e1i, dtype=np.int64), 'e2i': np.asarray(e2i, dtype=np.int64),
          'graph_per_obj_count': np.stack([ns_all, counts - ns_all], axis=1)}
    return {'emb': np.concatenate(rows), 'D': D, 'nnz': nnz, 'counts': counts, 'offs': offs, 'ns': ns_all, 'na': na_all,
            'data_dict': dd}


# ---- the same similarity three ways ------------------------------------------------------------------------------------
def pair_sim(e):
    """1 - (e/|e|)(e/|e|)^T in the precision of `e`."""
    e = e / np.sqrt((e * e).sum(axis=1))[:, None]
    return 1 - e @ e.T


def pair_sim_f32_emulation(e):
    """The fp32 kernels' formula in numpy fp32: 1 - ((a ia) . b) ib with ia = 1/sqrt(sum a^2)."""
    a = e.astype(np.float32)
    inv = np.float32(1) / np.sqrt((a * a).sum(axis=1, dtype=np.float32))
    return np.float32(1) - ((a * inv[:, None]) @ a.T) * inv[None, :]


def pair_sim_f16_emulation(e):
    """The fp16 routes: both operands are the normalised rows rounded to fp16, products and sums in fp32."""
    a = e.astype(np.float32)
    inv = np.float32(1) / np.sqrt((a * a).sum(axis=1, dtype=np.float32))
    h = (a * inv[:, None]).astype(np.float16).astype(np.float32)
    return np.float32(1) - h @ h.T


# ---- the reference -----------------------------------------------------------------------------------------------------
def case_sim(case, b):
    """The fp64 similarity block of pair b (computed once per case)."""
    sims = case.setdefault('_sims', {})
    if b not in sims:
        sims[b] = pair_sim(case['emb'][int(case['offs'][b]):int(case['offs'][b + 1])])
    return sims[b]


def others_in_order(sim_row, self_idx, reverse_ties=False):
    """The other objects of the pair by ascending distance, the self entry removed by value; ties by ascending index (a stable
    sort) -- or, with reverse_ties, by DESCENDING index: what a kernel with an inverted tie comparison would produce."""
    n = len(sim_row)
    order = np.lexsort((-np.arange(n), sim_row)) if reverse_ties else np.argsort(sim_row, kind='stable')
    return [int(j) for j in order if int(j) != self_idx]


def ref_simrank(case, q_idx, q_tgt, k, reverse_ties=False):
    """What ops.simrank returns for these queries: rank [Q] (1-based, -1 without a target in the pair), the k nearest other
    objects (pair-local, -1 past the end) and their distances (fp64, inf past the end)."""
    offs = case['offs']
    Q = len(q_idx)
    rank = np.full(Q, -1, dtype=np.int64)
    idx = np.full((Q, k), -1, dtype=np.int64)
    dist = np.full((Q, k), np.inf)
    for q in range(Q):
        g = int(q_idx[q])
        b = int(np.searchsorted(offs, g, side='right')) - 1
        o, n = int(offs[b]), int(offs[b + 1] - offs[b])
        row = case_sim(case, b)[g - o]
        order = others_in_order(row, g - o, reverse_ties)
        if q_tgt is not None and o <= int(q_tgt[q]) < o + n:
            rank[q] = order.index(int(q_tgt[q]) - o) + 1
        m = min(k, len(order))
        idx[q, :m] = order[:m]
        dist[q, :m] = row[order[:m]]
    return rank, idx, dist


def ref_pair_metrics(case, reverse_ties=False, reverse_sgar_order=None):
    """[B,12] like sga_pair_metrics: Hits@1..5 counts, #anchors, sum of reciprocal ranks (a target outside the pair adds
    nothing), SGAR '2' / '50' / '100' (the anchors' top-1 predictions by ascending distance, ties by anchor order; a mode holds
    when all of the first 2 / first half / all are right -- vacuously for no anchors), 0, 0.
    reverse_sgar_order (default: as reverse_ties) reverses the tie-break of the SGAR order alone."""
    reverse_sgar_order = reverse_ties if reverse_sgar_order is None else reverse_sgar_order
    dd = case['data_dict']
    rank, idx, dist = ref_simrank(case, dd['e1i'], dd['e2i'], 1, reverse_ties)
    out = np.zeros((len(case['counts']), 12))
    p = 0
    for b, na in enumerate(case['na']):
        na, o = int(na), int(case['offs'][b])
        r, pred, d = rank[p:p + na], idx[p:p + na, 0], dist[p:p + na, 0]
        gt = dd['e2i'][p:p + na] - o
        for k in range(5):
            out[b, k] = int(((r >= 1) & (r <= k + 1)).sum())
        out[b, 5] = na
        out[b, 6] = sum(1.0 / x for x in r if x >= 1)
        srt = np.lexsort((-np.arange(na), d)) if reverse_sgar_order else np.argsort(d, kind='stable')
        right = (pred == gt) & (pred >= 0)
        for c, sel in ((7, srt[:2]), (8, srt[:na // 2]), (9, srt)):
            out[b, c] = 1.0 if all(right[i] for i in sel) else 0.0
        p += na
    return out, rank


def ref_evaluate(case, reg_k=0, reverse_ties=False):
    """alignment.evaluate_batch's meter dict from the reference above (mrr as reciprocal ranks in fp64, 0 for a target outside
    its pair; SGAR lists without the anchor-less pairs)."""
    pm, rank = ref_pair_metrics(case, reverse_ties)
    res = {'mrr': [1.0 / r if r >= 1 else 0.0 for r in rank], 'ranks': rank,
           'sgar': {m: pm[case['na'] > 0, c].tolist() for m, c in (('2', 7), ('50', 8), ('100', 9))}}
    for k in (1, 2, 3, 4, 5):
        res[k] = {'correct': int(pm[:, k - 1].sum()), 'total': int(case['na'].sum())}
    if reg_k > 0:
        res['node_corrs'] = []
        for b, ns in enumerate(case['ns']):
            o, ns = int(case['offs'][b]), int(ns)
            _, idx, _ = ref_simrank(case, np.arange(o, o + ns), None, reg_k, reverse_ties)
            res['node_corrs'].append([(i, int(j)) for i in range(ns) for j in idx[i] if j >= ns])
    return res


# ---- how much the tie-break decides (conditions on the inputs, checked by test_simrank_cases_cpu.py) ------------------------
def tie_census(case, k=5):
    """Counts over the case: anchors (with a target in their pair) that have a third object exactly tied with the target, split by
    whether a tied object has a lower / a higher index than the target; queries (all objects) with an exact tie among their
    k+1 nearest; and whether some pair has two anchors with the same top-1 distance of which one is right and one is wrong."""
    dd, offs = case['data_dict'], case['offs']
    tied = tied_lower = tied_higher = anchors = 0
    for a, t in zip(dd['e1i'], dd['e2i']):
        b = int(np.searchsorted(offs, a, side='right')) - 1
        o, n = int(offs[b]), int(offs[b + 1] - offs[b])
        if not o <= t < o + n:
            continue
        anchors += 1
        row = case_sim(case, b)[a - o]
        j = np.flatnonzero(row == row[t - o])
        j = j[(j != a - o) & (j != t - o)]
        tied += bool(j.size)
        tied_lower += bool((j < t - o).any())
        tied_higher += bool((j > t - o).any())
    near = queries = 0
    for b, n in enumerate(case['counts']):
        o, n = int(offs[b]), int(n)
        sim = case_sim(case, b)
        for i in range(n):
            d = np.sort(np.delete(sim[i], i))[:k + 1]
            near += bool((d[1:] == d[:-1]).any())
            queries += 1
    _, idx, dist = ref_simrank(case, dd['e1i'], dd['e2i'], 1)
    mixed = False
    p = 0
    for b, na in enumerate(case['na']):
        na, o = int(na), int(offs[b])
        right = idx[p:p + na, 0] == dd['e2i'][p:p + na] - o
        d = dist[p:p + na, 0]
        mixed = mixed or any(right[i] != right[j] and d[i] == d[j] for i in range(na) for j in range(i))
        p += na
    return {'anchors': anchors, 'tied': tied, 'tied_lower': tied_lower, 'tied_higher': tied_higher, 'queries': queries,
            'near_tie': near, 'mixed_top1_tie': mixed}


# ---- the cases of tests/test_simrank_exact_gpu.py (D, pair sizes, seed); test_simrank_cases_cpu.py holds each to the conditions --
ROUTE_DIMS = (7, 16, 112, 113, 208, 209, 320, 321, 416, 417, 419, 430, 1000, 1024)
ROUTE_SIZES = (130, 8, 37, 11)         # two anchors each in the pairs of 8 (equal f) and 11
ROUTE_SEEDS = {**{D: 0 for D in ROUTE_DIMS}, 7: 6, 16: 2, 321: 2, 419: 2, 430: 2}
EDGE_SIZES = (512, 1, 2, 15, 16, 17, 63, 64, 65, 129, 511)
EDGE_ANCHORS = (170, 0, 0, 2, 2, 3, 20, 21, 21, 42, 170)
EDGE_DIMS = (416, 417, 1000)
EDGE_SEEDS = {D: 1 for D in EDGE_DIMS}
METRIC_SIZES = (40, 8, 8, 12, 200, 260, 512)
METRIC_ANCHORS = (0, 1, 2, 3, 64, 65, 200)
METRIC_D, METRIC_SEED = 300, 0

_made = {}


def route_case(D):
    return _cached(('route', D), lambda: make_case(D, ROUTE_SIZES, ROUTE_SEEDS[D], equal_f=(1,)))


def edge_case(D):
    return _cached(('edge', D), lambda: make_case(D, EDGE_SIZES, EDGE_SEEDS[D], anchors=EDGE_ANCHORS, lone_anchor_pair=1, equal_f=(3,)))


def metric_case():
    return _cached(('metric',), lambda: make_case(METRIC_D, METRIC_SIZES, METRIC_SEED, anchors=METRIC_ANCHORS, equal_f=(2,)))


def _cached(key, make):
    if key not in _made:
        _made[key] = make()
    return _made[key]


ALL_CASES = [('route', D) for D in ROUTE_DIMS] + [('edge', D) for D in EDGE_DIMS] + [('metric', METRIC_D)]


def get_case(kind, D):
    return route_case(D) if kind == 'route' else edge_case(D) if kind == 'edge' else metric_case()
