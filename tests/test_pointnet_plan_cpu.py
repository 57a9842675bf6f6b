"""CPU: the PointNet launcher's decision, written down.  sga_pointnet_plan is the function the launches themselves run (one copy of the conditions
in csrc/pointnet.hip); with a CU count passed in it touches no device, so the table below pins every launch form, every threshold and every size
on a machine without a card.  A threshold change edits this table on purpose.

Where the numbers come from: the launcher had no query before this file existed, so the table was derived by hand, by reading the launch code
of the commit before it (launch_fwd and sga_pointnet_bwd) -- not by running the plan and copying what it said:
    wave grid  g = min(ceil(T / 8), CUs)                    split = workspace >= 64 T C3 bytes and T < 4 CUs and P > 32
    mode 0     split: min(T, CUs) workgroups + combine, else g;  LDS (8192 + 128 C3) x 4
    mode 4     C3 = 256, not split, workspace >= 81 920: l-plane preparation on 20 workgroups, then g with 163 840 bytes of LDS (LG)
               else h = 2 at C3 = 256 (1 otherwise): h min(split ? T : g, h == 2 ? max(CUs / 2, 1) : CUs) workgroups, LDS (3072 + 1536 C3 / 32 / h) x 16
    BN sums    g' = the form's own grid: g' x 8 x (17 + C3 / 16) x 512 bytes zeroed, point moments on g', reduce on 265 + 2 C3 workgroups
    backward   mode 0: 2 T < CUs ? 2 T : CUs & ~1, LDS 99 840;  mode 4: 4 T < CUs ? 4 T : CUs & ~3, LDS 103 936"""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LG = 81920                               # the l planes of W2 and W3 at C3 = 256: (1024 + 8 x 512) x 16 bytes
ODD = 75                                 # a CU count that is no multiple of 2 or 4: CUs / 2 = 37, CUs & ~1 = 74, CUs & ~3 = 72, 4 CUs = 300
F32_LDS = {64: 65536, 128: 98304, 256: 163840}
P3_LDS = {64: 98304, 128: 147456, 256: 147456}
LG_LDS = 163840
BN_WG = {64: 86016, 128: 102400, 256: 135168}             # BatchNorm partials per workgroup: 8 waves x (17 + C3 / 16) slots x 64 lanes x 8 bytes
NO_AUX = (0, 0, 0, 0)


def part(T, C3):
    """The partials buffer: T objects x 8 waves x C3 channels x (value, index)."""
    return T * 8 * C3 * 8


def fwd(form, wgs, lds, ws_use='NONE', ws_used=0, bn=0, aux=NO_AUX):
    return (form, wgs, lds, ws_use, ws_used, bn, *aux)


# (pass, T, P, C3, mode, workspace bytes offered) -> the plan at 256 CUs | at ODD CUs (None: the same)
#   plan = (form, workgroups, LDS bytes, workspace use, workspace bytes used, bn_workspace bytes zeroed, l-plane prep, combine, point moments, reduce)
TABLE = [
    # T = 1023 | 1024 = 4 x 256 CUs, a partials-sized workspace: the split ends (at ODD CUs it ended at 300: one wave per object, LG on the buffer)
    (('FWD', 1023, 33, 256, 0, part(1023, 256)), fwd('F32_SPLIT', 256, 163840, 'PARTIALS', part(1023, 256), aux=(0, 1023, 0, 0)), fwd('F32_WAVE', 75, 163840)),
    (('FWD', 1024, 33, 256, 0, part(1024, 256)), fwd('F32_WAVE', 128, 163840), fwd('F32_WAVE', 75, 163840)),
    (('FWD', 1023, 33, 256, 4, part(1023, 256)), fwd('P3_SPLIT', 256, 147456, 'PARTIALS', part(1023, 256), aux=(0, 1023, 0, 0)),
     fwd('P3_LG', 75, LG_LDS, 'LG', LG, aux=(20, 0, 0, 0))),
    (('FWD', 1024, 33, 256, 4, part(1024, 256)), fwd('P3_LG', 128, LG_LDS, 'LG', LG, aux=(20, 0, 0, 0)), fwd('P3_LG', 75, LG_LDS, 'LG', LG, aux=(20, 0, 0, 0))),
    # the same threshold at ODD CUs: T = 299 | 300; the two-halves split runs 2 x (75 / 2) workgroups
    (('FWD', 299, 33, 256, 4, part(299, 256)), fwd('P3_SPLIT', 256, 147456, 'PARTIALS', part(299, 256), aux=(0, 299, 0, 0)),
     fwd('P3_SPLIT', 74, 147456, 'PARTIALS', part(299, 256), aux=(0, 299, 0, 0))),
    (('FWD', 300, 33, 256, 4, part(300, 256)), fwd('P3_SPLIT', 256, 147456, 'PARTIALS', part(300, 256), aux=(0, 300, 0, 0)),
     fwd('P3_LG', 38, LG_LDS, 'LG', LG, aux=(20, 0, 0, 0))),
    (('FWD', 299, 33, 256, 0, part(299, 256)), fwd('F32_SPLIT', 256, 163840, 'PARTIALS', part(299, 256), aux=(0, 299, 0, 0)),
     fwd('F32_SPLIT', 75, 163840, 'PARTIALS', part(299, 256), aux=(0, 299, 0, 0))),
    # P = 32 | 33 at T = 9: one 32-point tile per object is never split -- in mode 4 at C3 = 256 the partials buffer then serves as LG scratch
    (('FWD', 9, 32, 256, 0, part(9, 256)), fwd('F32_WAVE', 2, 163840), None),
    (('FWD', 9, 33, 256, 0, part(9, 256)), fwd('F32_SPLIT', 9, 163840, 'PARTIALS', part(9, 256), aux=(0, 9, 0, 0)), None),
    (('FWD', 9, 32, 256, 4, part(9, 256)), fwd('P3_LG', 2, LG_LDS, 'LG', LG, aux=(20, 0, 0, 0)), None),
    (('FWD', 9, 33, 256, 4, part(9, 256)), fwd('P3_SPLIT', 18, 147456, 'PARTIALS', part(9, 256), aux=(0, 9, 0, 0)), None),
    (('FWD', 9, 32, 128, 4, part(9, 128)), fwd('P3', 2, 147456), None),
    (('FWD', 9, 33, 128, 4, part(9, 128)), fwd('P3_SPLIT', 9, 147456, 'PARTIALS', part(9, 128), aux=(0, 5, 0, 0)), None),
    (('FWD', 9, 33, 64, 4, part(9, 64)), fwd('P3_SPLIT', 9, 98304, 'PARTIALS', part(9, 64), aux=(0, 3, 0, 0)), None),
    # a workspace one byte short of the partials (147 455 bytes at C3 = 256 are still LG scratch), and one byte short of the LG scratch
    (('FWD', 9, 33, 256, 0, part(9, 256) - 1), fwd('F32_WAVE', 2, 163840), None),
    (('FWD', 9, 33, 256, 4, part(9, 256) - 1), fwd('P3_LG', 2, LG_LDS, 'LG', LG, aux=(20, 0, 0, 0)), None),
    (('FWD', 9, 33, 128, 4, part(9, 128) - 1), fwd('P3', 2, 147456), None),
    (('FWD', 1100, 33, 256, 4, LG - 1), fwd('P3', 256, 147456), fwd('P3', 74, 147456)),
    (('FWD', 1100, 33, 256, 4, LG), fwd('P3_LG', 138, LG_LDS, 'LG', LG, aux=(20, 0, 0, 0)), fwd('P3_LG', 75, LG_LDS, 'LG', LG, aux=(20, 0, 0, 0))),
    # T = 3 at C3 = 256 with its partials buffer (49 152 bytes: no LG scratch) and P <= 32: the two halves of one object
    (('FWD', 3, 31, 256, 4, part(3, 256)), fwd('P3', 2, 147456), None),
    # T = 1100 for each C3 (138 workgroups of 8 objects), no workspace
    (('FWD', 1100, 33, 64, 0, 0), fwd('F32_WAVE', 138, 65536), fwd('F32_WAVE', 75, 65536)),
    (('FWD', 1100, 33, 128, 0, 0), fwd('F32_WAVE', 138, 98304), fwd('F32_WAVE', 75, 98304)),
    (('FWD', 1100, 33, 256, 0, 0), fwd('F32_WAVE', 138, 163840), fwd('F32_WAVE', 75, 163840)),
    (('FWD', 1100, 33, 64, 4, 0), fwd('P3', 138, 98304), fwd('P3', 75, 98304)),
    (('FWD', 1100, 33, 128, 4, 0), fwd('P3', 138, 147456), fwd('P3', 75, 147456)),
    (('FWD', 1100, 33, 256, 4, 0), fwd('P3', 256, 147456), fwd('P3', 74, 147456)),
    # every form with the BatchNorm sums: the form's own grid sizes the zeroed partials and the point moments
    (('FWD_BN', 1100, 33, 64, 0, 0), fwd('F32_WAVE', 138, 65536, bn=11870208, aux=(0, 0, 138, 393)), fwd('F32_WAVE', 75, 65536, bn=6451200, aux=(0, 0, 75, 393))),
    (('FWD_BN', 9, 33, 256, 0, part(9, 256)), fwd('F32_SPLIT', 9, 163840, 'PARTIALS', part(9, 256), bn=1216512, aux=(0, 9, 9, 777)), None),
    (('FWD_BN', 1100, 33, 128, 4, 0), fwd('P3', 138, 147456, bn=14131200, aux=(0, 0, 138, 521)), fwd('P3', 75, 147456, bn=7680000, aux=(0, 0, 75, 521))),
    (('FWD_BN', 3, 31, 256, 4, part(3, 256)), fwd('P3', 2, 147456, bn=270336, aux=(0, 0, 2, 777)), None),
    (('FWD_BN', 9, 33, 256, 4, part(9, 256)), fwd('P3_SPLIT', 18, 147456, 'PARTIALS', part(9, 256), bn=2433024, aux=(0, 9, 18, 777)), None),
    (('FWD_BN', 1100, 33, 256, 4, LG), fwd('P3_LG', 138, LG_LDS, 'LG', LG, bn=18653184, aux=(20, 0, 138, 777)),
     fwd('P3_LG', 75, LG_LDS, 'LG', LG, bn=10137600, aux=(20, 0, 75, 777))),
    (('FWD_BN', 9, 32, 256, 4, part(9, 256)), fwd('P3_LG', 2, LG_LDS, 'LG', LG, bn=270336, aux=(20, 0, 2, 777)), None),
    # backward: quadruples (mode 4) on both sides of 4 T = CUs, pairs (mode 0) on both sides of 2 T = CUs
    (('BWD', 63, 40, 256, 4, 0), fwd('BWD_P3', 252, 103936), fwd('BWD_P3', 72, 103936)),
    (('BWD', 64, 40, 256, 4, 0), fwd('BWD_P3', 256, 103936), fwd('BWD_P3', 72, 103936)),
    (('BWD', 65, 40, 256, 4, 0), fwd('BWD_P3', 256, 103936), fwd('BWD_P3', 72, 103936)),
    (('BWD', 18, 40, 256, 4, 0), fwd('BWD_P3', 72, 103936), None),
    (('BWD', 19, 40, 256, 4, 0), fwd('BWD_P3', 76, 103936), fwd('BWD_P3', 72, 103936)),
    (('BWD', 127, 40, 256, 0, 0), fwd('BWD_F32', 254, 99840), fwd('BWD_F32', 74, 99840)),
    (('BWD', 128, 40, 256, 0, 0), fwd('BWD_F32', 256, 99840), fwd('BWD_F32', 74, 99840)),
    (('BWD', 37, 1, 256, 0, 0), fwd('BWD_F32', 74, 99840), None),
    (('BWD', 38, 1, 256, 0, 0), fwd('BWD_F32', 76, 99840), fwd('BWD_F32', 74, 99840)),
    # nothing to do: a zero-object shard (the forward does not look at C3 then, as before)
    (('FWD', 0, 5, 256, 4, LG), fwd('EMPTY', 0, 0), None),
    (('FWD_BN', 0, 5, 100, 0, 0), fwd('EMPTY', 0, 0), None),
    (('BWD', 0, 5, 256, 4, 0), fwd('EMPTY', 0, 0), None),
]


def _plan(args, ncu):
    from sgaligner_amd import ops
    which, T, P, C3, mode, ws = args
    return tuple(ops.pointnet_plan(which, T, P, C3, mode, ws_bytes=ws, ncu=ncu))


def _id(row):
    return '-'.join(str(a) for a in row[0])


@pytest.mark.parametrize('row', TABLE, ids=_id)
def test_launch_table(row):
    args, at256, at_odd = row
    assert _plan(args, 256) == at256, '256 CUs'
    assert _plan(args, ODD) == (at_odd or at256), f'{ODD} CUs'


def test_table_is_consistent_with_its_own_constants():
    """The table's literals against the formulas of the module text (a typo in one of them must not pass as a pinned value)."""
    assert LG == (1024 + 8 * 512) * 16
    for args, at256, at_odd in TABLE:
        which, T, P, C3, mode, ws = args
        for ncu, (form, wgs, lds, use, used, bn, prep, comb, xm, red) in ((256, at256), (ODD, at_odd or at256)):
            if form == 'EMPTY':
                continue
            assert lds == {'F32_WAVE': F32_LDS[C3], 'F32_SPLIT': F32_LDS[C3], 'P3': P3_LDS[C3], 'P3_SPLIT': P3_LDS[C3], 'P3_LG': LG_LDS, 'BWD_F32': 99840,
                           'BWD_P3': 103936}[form], args
            assert (use, used) == {'F32_SPLIT': ('PARTIALS', part(T, C3)), 'P3_SPLIT': ('PARTIALS', part(T, C3)), 'P3_LG': ('LG', LG)}.get(form, ('NONE', 0)), args
            assert prep == (20 if form == 'P3_LG' else 0) and comb == (-(-T * C3 // 256) if form.endswith('SPLIT') else 0), args
            assert (bn, xm, red) == ((wgs * BN_WG[C3], wgs, 265 + 2 * C3) if which == 'FWD_BN' else (0, 0, 0)), args
            assert wgs <= max(ncu, 2)


def test_table_holds_every_form_and_bn_with_every_forward_form():
    from sgaligner_amd import _lib
    seen = {r[1][0] for r in TABLE} | {r[2][0] for r in TABLE if r[2]}
    assert seen | {'REFUSED'} == set(_lib.POINTNET_FORMS), set(_lib.POINTNET_FORMS) ^ seen
    bn = {r[1][0] for r in TABLE if r[0][0] == 'FWD_BN'}
    assert bn >= {'F32_WAVE', 'F32_SPLIT', 'P3', 'P3_SPLIT', 'P3_LG'}


def test_names_are_the_header_enums():
    from sgaligner_amd import _lib
    txt = open(os.path.join(ROOT, 'include', 'sgaligner_hip.h')).read()
    txt = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    for enum, prefix, names in (('sga_pointnet_form', 'SGA_POINTNET_', _lib.POINTNET_FORMS), ('sga_pointnet_pass', 'SGA_POINTNET_', _lib.POINTNET_PASSES),
                                ('sga_pointnet_ws_use', 'SGA_POINTNET_WS_', _lib.POINTNET_WS_USES)):
        body = re.search(r'enum\s+%s\s*\{(.*?)\}' % enum, txt, flags=re.S).group(1)
        assert tuple(re.findall(prefix + r'(\w+)', body)) == names, enum
    assert int(re.search(r'#define\s+SGA_POINTNET_PLAN_FIELDS\s+(\d+)', txt).group(1)) == _lib.POINTNET_PLAN_FIELDS
    assert _lib.lib().sga_version() >= 104
    assert _lib.lib().sga_pointnet_fwd_lg_ws_bytes() == LG


def _sweep():
    for T in range(1, 2101):
        for C3 in (64, 128, 256):
            for mode in (0, 4):
                for ws in (0, LG, part(T, C3)):
                    for P in (1, 33):
                        yield T, P, C3, mode, ws


def test_bn_workspace_bound_holds_for_every_form():
    """sga_pointnet_fwd_bn_ws_bytes(T, C3) -- what the caller allocates -- is never less than what the planned form zeroes, on this machine's CU
    count (the bound asks the device; without one the library plans for 256)."""
    from sgaligner_amd import _lib
    l = _lib.lib()
    ncu = int(l.sga_device_cus())
    out = (ctypes.c_int32 * _lib.POINTNET_PLAN_FIELDS)()
    bound = {(T, C3): int(l.sga_pointnet_fwd_bn_ws_bytes(T, C3)) for T in range(1, 2101) for C3 in (64, 128, 256)}
    for T, P, C3, mode, ws in _sweep():
        assert l.sga_pointnet_plan(1, T, P, C3, mode, ws, ncu, out) == 0
        assert 0 < out[5] <= bound[T, C3], (T, P, C3, mode, ws, ncu, list(out))
        assert out[5] == out[1] * BN_WG[C3] and out[8] == out[1]


@pytest.mark.parametrize('ncu', [256, ODD, 304, 2])
def test_workspace_used_never_exceeds_the_workspace_offered(ncu):
    from sgaligner_amd import _lib
    l = _lib.lib()
    out = (ctypes.c_int32 * _lib.POINTNET_PLAN_FIELDS)()
    for T, P, C3, mode, ws in _sweep():
        for which in (0, 1):
            assert l.sga_pointnet_plan(which, T, P, C3, mode, ws, ncu, out) == 0
            assert out[4] <= ws and (out[4] == 0) == (out[3] == 0), (which, T, P, C3, mode, ws, ncu, list(out))
            assert 1 <= out[1] <= ncu


def test_workspace_the_python_layer_offers():
    """pointnet_forward's half of the rule (pointnet_ops.pointnet_workspace_bytes): a partials buffer up to POINTNET_SPLIT_MAX_OBJECTS objects, LG
    scratch above that in mode 4 at C3 = 256, nothing otherwise."""
    from sgaligner_amd import ops
    assert ops.POINTNET_SPLIT_MAX_OBJECTS == 1023
    assert ops.pointnet_workspace_bytes(9, 256, 4) == part(9, 256) and ops.pointnet_workspace_bytes(1023, 64, 0) == part(1023, 64)
    assert ops.pointnet_workspace_bytes(1024, 256, 4) == LG and ops.pointnet_workspace_bytes(1024, 256, 0) == 0
    assert ops.pointnet_workspace_bytes(1024, 128, 4) == 0 and ops.pointnet_workspace_bytes(0, 256, 4) == 0
    keep = ops.POINTNET_SPLIT_MAX_OBJECTS
    try:
        ops.POINTNET_SPLIT_MAX_OBJECTS = 0
        assert ops.pointnet_workspace_bytes(9, 256, 4) == LG and ops.pointnet_workspace_bytes(9, 256, 0) == 0
    finally:
        ops.POINTNET_SPLIT_MAX_OBJECTS = keep


def test_plan_refuses_what_the_entry_points_refuse():
    """Bad arguments: SGA_ERR_ARG = 1, the form REFUSED, and the entry point's own message -- through the plan and through the entry points
    themselves (null pointers: nothing is dereferenced before the refusal)."""
    from sgaligner_amd import _lib
    l = _lib.lib()
    out = (ctypes.c_int32 * _lib.POINTNET_PLAN_FIELDS)()

    def refused(which, T, P, C3, mode, text, plan=out):
        assert l.sga_pointnet_plan(which, T, P, C3, mode, 0, 256, plan) == 1
        assert text in l.sga_last_error(), l.sga_last_error()
        if plan is not None:
            assert _lib.POINTNET_FORMS[plan[0]] == 'REFUSED' and list(plan[1:]) == [0] * 9

    for which in (0, 1):
        refused(which, 4, 0, 256, 0, b'sga_pointnet_fwd: need T >= 0 and P >= 1 (got T=4 P=0)')
        refused(which, -1, 8, 256, 0, b'sga_pointnet_fwd: need T >= 0 and P >= 1 (got T=-1 P=8)')
        refused(which, 4, 8, 100, 0, b'sga_pointnet_fwd: out_size C3=100 unsupported (64, 128 or 256: W3 must fit the 160 KiB LDS)')
    refused(0, 4, 8, 256, 3, b'sga_pointnet_fwd: mode 3 (0 = exact fp32, 4 = three exact bf16 planes)')
    refused(1, 4, 8, 256, 3, b'sga_pointnet_fwd_bn: mode 3 (0 = exact fp32, 4 = three exact bf16 planes)')
    refused(2, 4, 8, 128, 0, b'sga_pointnet_bwd: out_size C3=128 unsupported (256 only)')
    refused(2, 4, 8, 256, 1, b'sga_pointnet_bwd: mode 1 (0 = exact fp32 MFMA, 4 = three exact bf16 planes)')
    refused(2, 4, 0, 256, 0, b'sga_pointnet_bwd: bad sizes')
    refused(3, 4, 8, 256, 0, b'sga_pointnet_plan: pass 3')
    refused(0, 4, 0, 256, 0, b'P >= 1', plan=None)          # a null plan pointer only checks the arguments
    assert l.sga_pointnet_plan(0, 4, 8, 256, 0, 0, 256, None) == 0

    n9, n15 = (None,) * 9, (None,) * 15
    assert l.sga_pointnet_fwd_ws(*n9, 4, 8, 256, None, 0, 3, None) == 1 and b'sga_pointnet_fwd: mode 3' in l.sga_last_error()
    assert l.sga_pointnet_fwd_ws(*n9, 4, 8, 256, None, 0, 4, None) == 1 and b'sga_pointnet_fwd: null pointer' in l.sga_last_error()
    assert l.sga_pointnet_fwd_bn(*n9, 4, 8, 256, None, 0, None, 0, None, 0, None) == 1 and b'sga_pointnet_fwd_bn: bn_sums is null' in l.sga_last_error()
    assert l.sga_pointnet_bwd(*n15, 4, 8, 128, 0, None) == 1 and b'(256 only)' in l.sga_last_error()
    assert l.sga_pointnet_bwd(*n15, 4, 8, 256, 4, None) == 1 and b'sga_pointnet_bwd: null pointer' in l.sga_last_error()
