"""GPU: the attention kernels of 2 heads x 128 channels (width and head count literal) against the general, run-time-width kernels,
exactly.  A 2 x 128 case is re-laid at 2 x 129 with an all-zero 129th channel in H, att_src, att_dst, bias and the cotangent: the
run-time launch at C = 129 then performs the same operations in the same order plus exact zeros (a zero term of every dot product, a zero
column that is copied, aggregated and written).  All values are integers in [-2, 2] scaled by 2^-3, so that
the logits' node parts, which the two kernel families sum in a different association, are exact in both."""
import pytest
import torch

import gat_general_gate as GG

pytestmark = pytest.mark.gpu

SIZES = (5, 64, 129)            # the 64-node graph is complete
CAPS = (129, 64)                # the launches: all three graphs (NJ = 4), and those of at most 64 nodes (NJ = 2); the 129-node launch reads features from global memory at 128 and from LDS at 129


def _lattice(gen, *shape):
    return torch.randint(-2, 3, shape, generator=gen).float() / 8.0


def _relay(a):
    """[.., 2 * 128] -> [.., 2 * 129], channel 128 of each head zero."""
    out = torch.zeros(a.shape[:-1] + (2 * 129,))
    for hd in range(2):
        out[..., hd * 129:hd * 129 + 128] = a[..., hd * 128:hd * 128 + 128]
    return out


def _real(a):
    return torch.cat([a[..., hd * 129:hd * 129 + 128] for hd in range(2)], -1)


@pytest.mark.parametrize('cap', CAPS)
def test_kernels_of_2x128_equal_run_time_width(cap):
    from sgaligner_amd import ops
    gen = torch.Generator().manual_seed(0)
    sizes = [n for n in SIZES if n <= cap]
    graphs = [(n, GG._complete(n), True) if n == 64 else (n, GG._random_pairs(n, gen), False) for n in sizes]
    gb = GG.graph_batch(graphs)
    assert gb.complete.cpu().tolist() == [int(n == 64) for n in sizes]
    T = sum(sizes)
    H, a_s, a_d, b, cot = _lattice(gen, T, 256), _lattice(gen, 256), _lattice(gen, 256), _lattice(gen, 256), _lattice(gen, T, 256)

    def run(channels, *ts):
        H, a_s, a_d, b, cot = [t.cuda().contiguous() for t in ts]
        out = ops._attn_fwd_hc(H, 2, channels, a_s, a_d, b, gb, check_status=True)
        dh, das, dad = ops._attn_bwd_hc(H, cot, 2, channels, a_s, a_d, gb)
        torch.cuda.synchronize()
        ops.DEFERRED_CHECKS.flush()
        return [t.cpu() for t in (out, dh, das, dad)]
    lit = run(128, H, a_s, a_d, b, cot)
    wide = run(129, *[_relay(t) for t in (H, a_s, a_d, b, cot)])
    assert all(torch.equal(w[..., 128::129], torch.zeros_like(w[..., 128::129])) for w in wide[:2])      # the padding column: bias 0, dH 0
    out, dh, das, dad = [_real(w) for w in wide]
    assert torch.equal(lit[0], out)
    # equal up to the order of the kernels' floating-point atomics (d a_s across a workgroup's waves, d att_* across graphs): test_stacks' bound
    for name, got, want in (('dH', lit[1], dh), ('d att_src', lit[2], das), ('d att_dst', lit[3], dad)):
        err, bound = (got - want).abs().max().item(), 1e-5 * max(1.0, want.abs().max().item())
        print(f'{name}: max |2x128 - run-time| {err:.3e}, bound {bound:.3e}')
        assert err <= bound, (name, err, bound)
