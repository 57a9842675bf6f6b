"""CPU tier of the pair-job contract (csrc/pair_jobs.h, sgaligner_amd/packed.py): the one chunk rule gives, through its three named
wrappers, the integers the three separate rules gave; PairJobs on a hand-written case and its refusals; the two searches and RANSAC
refuse a bad job list, chunk and workspace in the same words behind the C ABI, without a device."""
import numpy as np
import pytest


def _mixed(n, mul, add=0):
    """n sizes in [50, 2000], a fixed arithmetic sequence (no generator whose stream could change)."""
    return [50 + (i * mul + add) % 1951 for i in range(n)]


# (sizes of the axis that is tiled, sizes of the axis that is split) for _nn_chunk and _featnn_chunk: (queries, supports); _ransac_chunk
# takes the split axis first, so the same pairs read (rows, hypotheses) there.
CASES = [
    ([], []),                                                       # an empty list
    ([1], [1]), ([100], [100]), ([100], [127]),                     # one job below every minimum chunk (128, 1024, 2048)
    ([127], [128]), ([128], [129]), ([129], [1023]), ([1023], [1024]), ([1024], [1025]), ([1025], [2047]), ([2047], [2048]),
    ([2048], [2049]), ([4096], [4097]),
    ([10000], [10000]),                                             # one 10 000 x 10 000 job
    ([20000], [5000]),                                              # RANSAC: 20 000 rows x 5 000 hypotheses, the 785-workgroup grid
    ([5000], [20000]), ([20000], [20000]), ([50000], [50000]), ([200000], [200000]), ([1000000], [1000000]), ([1], [1000000]),
    ([1000000], [1]), ([0], [5000]), ([5000], [0]), ([0, 0], [0, 0]),
    ([50000] * 45, [50000] * 45),                                   # the C(10, 2) subscan pairs of a scan
    ([300, 0, 129, 5], [257, 10, 0, 100]), ([1025, 0, 129, 300], [300, 0, 129, 1025]),
    (_mixed(200, 977), _mixed(200, 1409, 7)),                       # 200 jobs of 50-2000 rows
    (_mixed(200, 1409, 7), _mixed(200, 977)),
    (_mixed(200, 977), [10000] * 200), ([10000] * 200, _mixed(200, 977)),
    ([10000] * 4, [10000] * 4), ([3000] * 10, [40000] * 10), ([130] * 300, [100000] * 300), ([20000] * 3, [5000] * 3),
    ([5000] * 7, [20000] * 7), ([999], [99999]), ([12345], [67890]), ([67890], [12345]), ([2 ** 20 + 1], [2 ** 20 + 1]),
    ([640], [3 * 2048 + 1]),
]

# What _nn_chunk, _featnn_chunk and _ransac_chunk returned for CASES, in order, before they shared split_chunk, with sga_device_cus
# stubbed to 256 and to 64: recorded on the commit before the rule was unified.
CHUNKS = {
    ('nn', 256): [2048, 2048, 2048, 2048, 2048, 2048, 2048, 2048, 2048, 2048, 2048, 2048, 2048, 2048,
                  2048, 2048, 2048, 2048, 9524, 200000, 2048, 2048, 2048, 2048, 2048, 25000, 2048, 2048,
                  2048, 2048, 2048, 2048, 2048, 2048, 7143, 2048, 2048, 2048, 2048, 2048, 262145, 2048],
    ('featnn', 256): [1024, 1024, 1024, 1024, 1024, 1024, 1024, 1024, 1024, 1024, 1024, 1024, 1024, 1024,
                      1024, 1024, 2944, 16768, 200064, 1000064, 1024, 1024, 1024, 1024, 1024, 50048, 1024, 1024,
                      2048, 1408, 10112, 1408, 2560, 8064, 50048, 1792, 5120, 1024, 6272, 6272, 1048704, 1024],
    ('ransac', 256): [128, 128, 128, 128, 128, 128, 128, 128, 128, 128, 128, 128, 128, 132,
                      131, 132, 131, 603, 10000, 250000, 128, 245, 128, 128, 128, 50000, 128, 128,
                      133, 154, 662, 770, 132, 300, 130, 131, 173, 143, 203, 216, 349526, 128],
    ('nn', 64): [2048, 2048, 2048, 2048, 2048, 2048, 2048, 2048, 2048, 2048, 2048, 2048, 2048, 2048,
                 2048, 2048, 2048, 2381, 33334, 500000, 2048, 2048, 2048, 2048, 2048, 50000, 2048, 2048,
                 2048, 2048, 2500, 2048, 2048, 2048, 25000, 2048, 2048, 2048, 2048, 2048, 1048577, 2048],
    ('featnn', 64): [1024, 1024, 1024, 1024, 1024, 1024, 1024, 1024, 1024, 1024, 1024, 1024, 1024, 2560,
                     2560, 2944, 10112, 50048, 200064, 1000064, 3968, 1024, 1024, 1024, 1024, 50048, 1024, 1024,
                     2048, 1408, 10112, 1408, 10112, 20096, 100096, 5120, 20096, 3200, 22656, 12416, 1048704, 1024],
    ('ransac', 64): [128, 128, 128, 128, 128, 128, 128, 128, 128, 128, 128, 128, 164, 132,
                     131, 132, 393, 2500, 40000, 1000000, 128, 977, 128, 128, 128, 50000, 128, 128,
                     442, 667, 1324, 3334, 400, 1500, 130, 295, 715, 143, 823, 871, 1048577, 128],
}


class _Cus:
    def __init__(self, cus):
        self.cus = cus

    def sga_device_cus(self):
        return self.cus


@pytest.mark.parametrize('cus', (256, 64))
def test_the_chunk_rule_is_unchanged(cus, monkeypatch):
    from sgaligner_amd import _lib
    from sgaligner_amd.utils import point_cloud as PC, registration as RG
    assert len(CASES) >= 40
    monkeypatch.setattr(_lib, 'lib', lambda: _Cus(cus))
    for name, fn in (('nn', PC._nn_chunk), ('featnn', RG._featnn_chunk), ('ransac', RG._ransac_chunk)):
        want = CHUNKS[name, cus]
        assert len(want) == len(CASES)
        got = [fn(a, b) for a, b in CASES]
        assert all(type(g) is int for g in got), name
        assert got == want, (name, cus, [(i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w])
        assert got == [fn(np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)) for a, b in CASES]      # as the callers pass them
    # 20 000 rows x 5 000 hypotheses on 256 CUs: 5 tiles x 153 chunks of 131 rows = 765 workgroups, three per CU at most, not 785
    assert CHUNKS['ransac', 256][CASES.index(([20000], [5000]))] == 131 == -(-20000 // 153)


def test_split_chunk_is_the_rule_the_wrappers_state():
    from sgaligner_amd.packed import split_chunk
    assert split_chunk(0, 0, 256, 16, 2048) == 2048                                  # nothing to split: the minimum
    assert split_chunk(10, 10000, 256, 16, 2048) == 2048                              # min(410, 5) chunks of 2000 rows: the minimum instead
    # 8 tiles on 64 CUs at 4 per CU: min(32, 98) chunks of ceil(100000 / 32) = 3125 rows, rounded up to whole tiles of 128
    assert split_chunk(8, 100000, 64, 4, 1024) == 3125 and split_chunk(8, 100000, 64, 4, 1024, round_to=128) == 3200
    # whole rounds: 5 tiles x 157 chunks = 785 workgroups on 256 CUs are trimmed to 153 chunks = 765 <= 768
    assert split_chunk(5, 20000, 256, 16, 128, whole_rounds=True) == -(-20000 // 153)
    assert split_chunk(5, 20000, 256, 16, 128) == -(-20000 // 157)


def test_pair_jobs_on_a_hand_written_case():
    from sgaligner_amd.packed import PairJobs
    J = PairJobs([0, 3, 3, 8, 10], 10, [(0, 2), (1, 0), (2, 1), (3, 3)], 'caller', 'set')
    assert J.n_sets == 4 and J.n_pairs == 4
    assert J.nq.tolist() == [3, 0, 5, 2] and J.ns.tolist() == [5, 3, 0, 2]
    assert J.out_off.tolist() == [0, 3, 3, 8, 10] and J.out_off.dtype == np.int64 and J.total_q == 10
    assert (J.max_q, J.max_s) == (5, 5)
    assert J.h_off.tolist() == [0, 3, 3, 8, 10] and J.h_pr.tolist() == [[0, 2], [1, 0], [2, 1], [3, 3]] and J.h_oo.tolist() == [0, 3, 3, 8]
    assert J.h_off.dtype == J.h_pr.dtype == J.h_oo.dtype == np.int32
    parts = J.host_parts()
    assert len(parts) == 3 and parts[0] is J.h_off and parts[1] is J.h_pr and parts[2] is J.h_oo
    assert all(p.flags['C_CONTIGUOUS'] for p in parts)
    E = PairJobs([0, 4], 4, np.zeros((0, 2), dtype=np.int64), 'caller', 'set')            # no job: nothing to take a maximum of
    assert (E.n_pairs, E.total_q, E.max_q, E.max_s) == (0, 0, 0, 0) and E.out_off.tolist() == [0]
    with pytest.raises(ValueError, match=r'^pairs must name sets in \[0, 4\)$'):
        PairJobs([0, 3, 3, 8, 10], 10, [(0, 4)], 'caller', 'set')                          # an id out of range
    with pytest.raises(ValueError, match=r'^pairs must name clouds in \[0, 4\)$'):
        PairJobs([0, 3, 3, 8, 10], 10, [(-1, 0)], 'caller', 'cloud')
    with pytest.raises(ValueError, match=r'^offsets must be a monotone prefix array starting at 0 and covering all 10 entries$'):
        PairJobs([0, 3, 2, 8, 10], 10, [(0, 2)], 'caller', 'set')                          # a non-monotone prefix
    with pytest.raises(ValueError, match=r'^offsets must be a monotone prefix array starting at 0 and covering all 11 entries$'):
        PairJobs([0, 3, 3, 8, 10], 11, [(0, 2)], 'caller', 'set')                          # a total mismatch
    with pytest.raises(ValueError, match=r'^caller indexes with int32: fewer than 2\^31 queries per call$'):
        PairJobs([0, 2 ** 20], 2 ** 20, np.zeros((2 ** 11, 2), dtype=np.int64), 'caller', 'set')


def test_hyp_jobs_on_a_hand_written_case_and_its_refusals(monkeypatch):
    """HypJobs with the device check waved through (dtype still checked first, as device_tensor does): the fields, and the refusals in the
    words find_rigid_transform_batch, edge_length_filter and hypothesis_models_batch gave before they shared it."""
    import torch
    from sgaligner_amd import packed
    from sgaligner_amd.packed import HypJobs
    corr, samples = torch.zeros((10, 6), dtype=torch.float64), torch.zeros((7, 3), dtype=torch.int32)
    with pytest.raises(RuntimeError, match=r'^sgaligner_amd: `corr` must be torch.float64 \(got torch.float32\)$'):       # dtype before device
        HypJobs(corr.float(), [0, 10], samples, [0, 7])
    with pytest.raises(RuntimeError, match=r'^sgaligner_amd: `corr` must be a HIP device tensor .*no CPU path'):
        HypJobs(corr, [0, 10], samples, [0, 7])
    monkeypatch.setattr(packed, 'device_tensor', lambda t, name, dtype: (packed.check_dtype(t, name, dtype), t.contiguous())[1])
    J = HypJobs(corr, [0, 4, 4, 10], samples, [0, 5, 5, 7])
    assert (J.n_jobs, J.total, J.total_h, J.max_n, J.max_h) == (3, 10, 7, 6, 5)
    assert J.sizes_n.tolist() == [4, 0, 6] and J.sizes_h.tolist() == [5, 0, 2]
    assert J.off.dtype == J.hoff.dtype == np.int64 and J.h_off.dtype == J.h_hoff.dtype == np.int32
    assert J.h_off.tolist() == [0, 4, 4, 10] and J.h_hoff.tolist() == [0, 5, 5, 7] and tuple(J.samples.shape) == (7, 3)
    E = HypJobs(corr[:0], [0], samples[:0], [0])                                           # no job: nothing to take a maximum of
    assert (E.n_jobs, E.total, E.total_h, E.max_n, E.max_h) == (0, 0, 0, 0, 0)
    with pytest.raises(RuntimeError, match=r'^sgaligner_amd: `samples` must be torch.int32 \(got torch.int64\)$'):
        HypJobs(corr, [0, 10], samples.long(), [0, 7])
    assert HypJobs(corr, [0, 10], samples.long().numpy(), [0, 7], convert_samples=True).samples.dtype == torch.int32
    with pytest.raises(ValueError, match=r'^corr must be \[N,6\], got \(12, 5\)$'):
        HypJobs(torch.zeros((12, 5), dtype=torch.float64), [0, 12], samples, [0, 7])
    assert HypJobs(torch.zeros((12, 5), dtype=torch.float64), [0, 12], samples, [0, 7], corr_shape=False).total == 12
    with pytest.raises(ValueError, match=r'^offsets must be a monotone prefix array starting at 0 and covering all 10 entries$'):
        HypJobs(corr, [0, 6, 4, 10], samples, [0, 5, 5, 7])                                # a non-prefix offsets
    with pytest.raises(ValueError, match=r'^hyp_offsets must be a monotone prefix array starting at 0 and covering all 7 entries$'):
        HypJobs(corr, [0, 4, 4, 10], samples, [0, 5, 5, 8])                                # a total that does not match
    with pytest.raises(ValueError, match=r'^offsets names 3 jobs, hyp_offsets 2$'):
        HypJobs(corr, [0, 4, 4, 10], samples, [0, 5, 7])                                   # unequal job counts
    J.check_int32('caller', 3)
    J.total_h = 2 ** 31 // 12
    J.check_int32('caller', 3)
    with pytest.raises(ValueError, match=r'^caller indexes with int32: fewer than 2\^31 / 6 rows and 2\^31 / 12 hypotheses per call$'):
        J.check_int32('caller', 12)


def test_pair_ids_is_the_pair_check_of_pair_jobs():
    from sgaligner_amd.packed import pair_ids
    pr = pair_ids([(0, 2), (1, 0)], 3, 'cloud')
    assert pr.dtype == np.int64 and pr.tolist() == [[0, 2], [1, 0]] and pair_ids(pr) is not None and pair_ids([]).shape == (0, 2)
    assert pair_ids([(0, 9)]).tolist() == [[0, 9]]                                         # without n_sets: the conversion alone
    with pytest.raises(ValueError, match=r'^pairs must name clouds in \[0, 2\)$'):
        pair_ids(pr, 2, 'cloud')


def test_resolve_chunk_and_workspace():
    import torch
    from sgaligner_amd.packed import resolve_chunk, workspace
    boom = lambda: 1 / 0                                                                   # the rule runs only when nothing else is given
    assert resolve_chunk(7, 5, boom) == 7 and resolve_chunk(None, 5, boom) == 5 and resolve_chunk(None, None, lambda: 3) == 3
    for arg in (0, -4):
        with pytest.raises(ValueError, match=rf'^chunk must be >= 1, got {arg}$'):
            resolve_chunk(arg, None, boom)
    with pytest.raises(ValueError, match=r'^chunk must be >= 1, got 0$'):
        resolve_chunk(None, 0, boom)
    for nbytes, words in ((0, 1), (1, 1), (8, 1), (9, 2), (80, 10)):
        w = workspace(nbytes, 'cpu')
        assert w.dtype == torch.float64 and tuple(w.shape) == (words,)


def _searches(l):
    """sga_nn_search / sga_featnn_search / sga_ransac_rigid on HOST memory that is never dereferenced: every call must stop before a
    launch.  -> three functions (kwargs -> error text with the entry point's name cut off)."""
    buf = np.zeros(64, dtype=np.float64)
    p = buf.ctypes.data
    keep = []

    def host(a):
        keep.append(np.ascontiguousarray(a, dtype=np.int32))
        return keep[-1].ctypes.data

    def text(rc, name, want_rc):
        msg = l.sga_last_error().decode()
        assert rc == want_rc and msg.startswith(name + ': '), (rc, msg)
        return msg[len(name) + 2:]

    def nn(off=(0, 4, 8), pairs=((0, 1),), max_q=4, max_s=4, chunk=1024, ws=True, rc=1):
        r = l.sga_nn_search(p, p, len(off) - 1, off[-1], p, len(pairs), p, 4, max_q, max_s, chunk, host(off), host(pairs), 0, p, p,
                            p if ws else None, 64 * 8 if ws else 0, None)
        return text(r, 'sga_nn_search', rc)

    def featnn(off=(0, 4, 8), pairs=((0, 1),), max_q=4, max_s=4, chunk=1024, ws=True, rc=1, tiles=((0, 0, 0),)):
        r = l.sga_featnn_search(p, 4, p, len(off) - 1, off[-1], p, len(pairs), p, p, len(tiles), 1, 4, max_q, max_s, chunk, host(off), host(pairs),
                                host(tiles), p, p, p if ws else None, 64 * 8 if ws else 0, None)
        return text(r, 'sga_featnn_search', rc)

    def ransac(ws_bytes):
        r = l.sga_ransac_rigid(p, p, 1, 16, p, p, 8, 16, 8, 128, host((0, 16)), host((0, 8)), 0.03, 2, p, p, p, p, p, p, p if ws_bytes else None,
                               ws_bytes, None)
        return text(r, 'sga_ransac_rigid', 3)

    return nn, featnn, ransac


def test_the_c_entries_refuse_in_the_same_words():
    from sgaligner_amd import _lib
    l = _lib.lib()
    nn, featnn, ransac = _searches(l)
    # a pair naming a missing set
    assert nn(pairs=((0, 2),)) == 'pair 0 names cloud (0, 2) of 2'
    assert featnn(pairs=((0, 2),)) == 'pair 0 names set (0, 2) of 2'
    assert nn(pairs=((0, 1), (-1, 0))).replace('cloud', 'set') == featnn(pairs=((0, 1), (-1, 0))) == 'pair 1 names set (-1, 0) of 2'
    # a pair larger than max_queries / max_support
    assert nn(max_q=3) == featnn(max_q=3) == 'pair 0 is larger than max_queries 3 / max_support 4'
    assert nn(max_s=3) == featnn(max_s=3) == 'pair 0 is larger than max_queries 4 / max_support 3'
    # chunk = 0, and the other shared argument check
    assert nn(chunk=0) == featnn(chunk=0) == 'chunk must be >= 1 (got 0)'
    assert nn(max_q=5) == featnn(max_q=5) == 'max_queries 5 exceeds total_queries 4'
    # a missing workspace: the split form of nn needs 2 chunks x 4 queries x 12 B; featnn the norms (8 rows x 4 B) + 2 x 4 x 8 B
    assert l.sga_nn_workspace_bytes(4, 4, 2) == 96 and l.sga_featnn_workspace_bytes(8, 4, 4, 2) == 96
    two = ((0, 0, 0), (0, 0, 1))
    assert nn(chunk=2, ws=False, rc=3) == featnn(chunk=2, ws=False, rc=3, tiles=two) == 'workspace of 96 bytes needed, 0 given'
    need = int(l.sga_ransac_workspace_bytes(1, 8, 16, 128))
    assert need > 0
    assert ransac(0) == f'workspace of {need} bytes needed, 0 given'
    assert ransac(need - 8) == f'workspace of {need} bytes needed, {need - 8} given'
