"""CPU (cross-compile only): every instantiation of the three-plane anchors x anchors kernel (csrc/anchor3.hip) runs two waves per SIMD --
at most 256 registers, nothing spilled -- and its own rows fit the CU's 160 KiB of LDS."""
import os
import re
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))


def test_anchor3_kernels_fit_two_waves_per_simd():
    import kernel_resources as kr
    from sgaligner_amd import _build
    if not os.path.exists(_build.HIPCC):
        pytest.skip('hipcc not available')
    src = os.path.join(_build.CSRC, 'anchor3.hip')
    assert '-fno-slp-vectorize' in _build.FILE_FLAGS['anchor3.hip']
    _, res = kr.analyse(src)
    ks = {k: v for k, v in res.items() if 'anchor3_bwd_kernel' in k}
    want = {f'anchor3_bwd_kernelILi{m}ELb{t}ELb{s}E' for m in (2, 3) for t, s in ((1, 1), (1, 0), (0, 0))}
    assert {w for w in want if any(w in k for k in ks)} == want, sorted(ks)
    text = open(src).read()
    nop = int(re.search(r'constexpr int A3_NOP = (\d+);', text).group(1))
    lds = re.search(r'constexpr size_t a3_lds_bytes\(int M\) \{ return \(size_t\)M \* 2 \* 2 \* A3_NOP \* 1024; \}', text)
    assert lds and 'a3_lds_bytes(M)}' in text[lds.end():], 'the launch computes its LDS some other way: update this test'
    for k, v in ks.items():
        m = int(re.search(r'anchor3_bwd_kernelILi(\d)E', k).group(1))
        print(k, v)
        assert v['vgpr'] + v['agpr'] <= 256 and v['occ'] >= 2, (k, v)
        assert v['scratch'] == 0 and v['vspill'] == 0 and v['sspill'] == 0, (k, v)
        assert not v.get('loop_scratch') and not v.get('loop_readlane'), (k, v)
        assert v['lds'] + m * 2 * 2 * nop * 1024 <= 160 * 1024, (k, v)
