"""PointNet object encoder -- drop-in for reference src/aligner/networks/pointnet.py:87-175
(`PointNetfeat`), forward/backward on the fused HIP kernels (csrc/pointnet.hip)."""
import torch
import torch.nn as nn

from ... import ops
from .base import BaseNetwork


class PointNetfeat(BaseNetwork):
    """Same constructor, attributes and state_dict keys as the reference class (pointnet.py:88-118):
    conv{1,2,3} are Conv1d(k=1) holders for the [out,in,1] weights; bn{1,2,3} exist because the reference
    creates (and checkpoints) them although their OUTPUT IS DISCARDED (pointnet.py:141-142,154-155,
    158-159) -- they never enter y and receive no gradient.

    HIP path: global_feat=True, input_transform=False, feature_transform=False (the only configuration
    the reference instantiates, sg_aligner.py:58).  Anything else raises.
    """

    def __init__(self, global_feat=True, input_transform=True, feature_transform=False, point_size=3, out_size=1024,
                 batch_norm=True, init_weights=True, pointnet_str=None):
        super().__init__()
        if input_transform or feature_transform or not global_feat or point_size != 3:
            raise NotImplementedError('sgaligner_amd PointNetfeat: only global_feat=True, input_transform=False, '
                                      'feature_transform=False, point_size=3 is implemented (sg_aligner.py:58)')
        self.name = 'pnetenc'
        self.use_batch_norm = batch_norm
        self.point_size = point_size
        self.out_size = out_size
        self.global_feat = global_feat
        self.input_transform = input_transform
        self.feature_transform = feature_transform
        self.conv1 = nn.Conv1d(point_size, 64, 1)
        self.conv2 = nn.Conv1d(64, 128, 1)
        self.conv3 = nn.Conv1d(128, out_size, 1)
        if batch_norm:
            self.bn1 = nn.BatchNorm1d(64)
            self.bn2 = nn.BatchNorm1d(128)
            self.bn3 = nn.BatchNorm1d(out_size)
        # The reference's discarded BN calls still update running_mean / running_var / num_batches_tracked in train mode
        # (pointnet.py:141-142,154-155,158-159).  The buffers never reach any output, but a checkpoint carries them, so the side effect is
        # reproduced by default: the forward kernel (either arithmetic) sums the batch statistics of the three pre-activations on its way
        # (sga_pointnet_fwd_bn, no second pass).  SGA_POINTNET_BN_STATS=0 (or this attribute) switches the side effect off.
        import os
        self.update_bn_running_stats = os.environ.get('SGA_POINTNET_BN_STATS', '1') != '0'
        if init_weights:                                     # pointnet.py:116-118
            self.init_weights('constant', 1, target_op='BatchNorm')
            self.init_weights('xavier_normal', 1)

    def forward(self, x, return_meta=False):
        """x [T,3,P] as in the reference (a permuted view of data_dict['tot_obj_pts'] [T,P,3])."""
        assert x.ndim > 2
        xt = x.permute(0, 2, 1)                               # -> [T,P,3]; free when x is the reference's view
        if not xt.is_contiguous():
            xt = xt.contiguous()
        side = self.training and self.use_batch_norm and self.update_bn_running_stats and xt.shape[0] * xt.shape[1] > 0
        # The kernels serve C3 in {64, 128, 256}.  Another out_size up to 256 (the EVA baseline's 200, eva.py:27) runs on the next one: conv3
        # gets zero rows on the device, the extra channels (all relu(0) = 0) and their statistics are cut off again, and autograd through
        # the pad and the slice hands conv3 its gradients.
        c3 = self.out_size
        c3k = next((c for c in (64, 128, 256) if c >= c3), c3)
        w3, b3 = self.conv3.weight, self.conv3.bias
        if c3k != c3:
            w3 = torch.cat([w3, w3.new_zeros((c3k - c3,) + tuple(w3.shape[1:]))])
            b3 = torch.cat([b3, b3.new_zeros(c3k - c3)])
        bn_sums = None
        if side and c3k in (64, 128, 256):
            bn_sums = torch.empty((265 + 2 * c3k,), device=xt.device, dtype=torch.float64)
        y = ops.pointnet(xt.float() if xt.dtype != torch.float32 else xt, self.conv1.weight, self.conv1.bias,
                         self.conv2.weight, self.conv2.bias, w3, b3, bn_sums=bn_sums)
        if c3k != c3:
            y = y[:, :c3]
            if bn_sums is not None:
                bn_sums = torch.cat([bn_sums[:265 + c3], bn_sums[265 + c3k:265 + c3k + c3]])
        if bn_sums is not None:
            self._fold_bn_sums(bn_sums, xt.shape[0] * xt.shape[1])
        elif side:
            self._update_bn_running_stats(xt)
        if return_meta:
            return y, torch.zeros([1]), torch.zeros([1])       # pointnet.py:138,151 dummies
        return y

    @torch.no_grad()
    def _fold_bn_sums(self, sums, n):
        """running_mean / running_var / num_batches_tracked of bn1..3 from the sums the forward kernel took (fp64 throughout):
        z1 = W1 x + b1 is affine in x, so its channel means / variances follow from the 9 point moments; z2 and z3 - b3 come as per-channel
        sum and sum of squares.  nn.BatchNorm1d semantics: momentum 0.1 (None: cumulative average), unbiased variance."""
        c3 = self.out_size
        m = sums[0:3] / n
        q = sums[3:9] / n
        m2 = torch.stack((q[0], q[1], q[2], q[1], q[3], q[4], q[2], q[4], q[5])).view(3, 3)
        cov = m2 - torch.outer(m, m)
        w1 = self.conv1.weight.detach().reshape(64, 3).double()
        mean1 = w1 @ m + self.conv1.bias.detach().double()
        var1 = ((w1 @ cov) * w1).sum(1)
        mean2 = sums[9:137] / n
        var2 = sums[137:265] / n - mean2 * mean2
        u = sums[265:265 + c3] / n
        var3 = sums[265 + c3:265 + 2 * c3] / n - u * u
        mean3 = u + self.conv3.bias.detach().double()
        unb = n / max(n - 1, 1)
        for bn, mean, var in ((self.bn1, mean1, var1), (self.bn2, mean2, var2), (self.bn3, mean3, var3)):
            bn.num_batches_tracked.add_(1)
            mom = bn.momentum
            if mom is None:                                   # cumulative moving average (nn.BatchNorm1d(momentum=None))
                mom_t = 1.0 / bn.num_batches_tracked.double()
                bn.running_mean.add_(((mean - bn.running_mean.double()) * mom_t).float())
                bn.running_var.add_(((var.clamp_min(0) * unb - bn.running_var.double()) * mom_t).float())
            else:
                bn.running_mean.mul_(1 - mom).add_(mean.float(), alpha=mom)
                bn.running_var.mul_(1 - mom).add_((var.clamp_min(0) * unb).float(), alpha=mom)

    @torch.no_grad()
    def _update_bn_running_stats(self, xt, chunk_rows=1 << 20):
        """Batch statistics of the three PRE-ReLU conv outputs over all T*P points, exactly what the reference's
        discarded bn1/bn2/bn3 calls fold into their buffers (momentum 0.1, unbiased variance).  HIP passes over
        point chunks: GEMM (+bias) -> per-channel sum / sum of squares (sga_bn_stats) -> ReLU in place."""
        from ... import _lib
        from ...ops import _p, _stream
        L = _lib.lib()
        rows = xt.reshape(-1, 3).float()
        n = rows.shape[0]
        convs = (self.conv1, self.conv2, self.conv3)
        bns = (self.bn1, self.bn2, self.bn3)
        sums = [torch.zeros(2 * c.weight.shape[0], device=rows.device, dtype=torch.float64) for c in convs]
        for r0 in range(0, n, chunk_rows):
            h = rows[r0:r0 + chunk_rows]
            for k, c in enumerate(convs):
                w = c.weight.reshape(c.weight.shape[0], -1)
                z = ops.gemm(h, w, False, True, h.shape[0], w.shape[0], w.shape[1], bias=c.bias)
                part = torch.empty_like(sums[k])
                _lib.check(L.sga_bn_stats(_p(z), z.stride(0), z.shape[0], z.shape[1], _p(part), _stream()), 'sga_bn_stats')
                sums[k] += part
                if k < 2:                                     # h = relu(z), in place (scale 1, shift 0)
                    one = torch.ones(z.shape[1], device=z.device)
                    zero = torch.zeros(z.shape[1], device=z.device)
                    _lib.check(L.sga_bn_apply(_p(z), z.stride(0), z.shape[0], z.shape[1], _p(one), _p(zero), 1, None, 0,
                                              _p(z), z.stride(0), _stream()), 'sga_bn_apply')
                h = z
        for k, bn in enumerate(bns):
            cch = bn.num_features
            mean = sums[k][:cch] / n
            var_unb = (sums[k][cch:] - n * mean * mean) / max(n - 1, 1)
            mom = 0.1 if bn.momentum is None else bn.momentum
            bn.running_mean.mul_(1 - mom).add_(mean.float(), alpha=mom)
            bn.running_var.mul_(1 - mom).add_(var_unb.clamp_min(0).float(), alpha=mom)
            bn.num_batches_tracked.add_(1)
