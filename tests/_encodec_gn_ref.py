"""CPU restatement of the ``time_group_norm`` EnCodec (the 48 kHz model) for shapes the numpy stand-in for MLX is too slow for (TEST HELPER, not product).

``oracle.encodec_ref.EncodecRef`` with ``nn.GroupNorm(1, C, pytorch_compatible=True)`` appended to every conv and transposed conv, as the reference's
``EncodecConv1d`` / ``EncodecConvTranspose1d`` do (codec/models/encodec/encodec.py:172-291): per sample, mean and biased variance over all (time x
channel) elements, eps 1e-5, then the per-channel ``<layer>.norm.weight`` / ``.norm.bias``; the transposed conv is normalised BEFORE its trim.
Everything else (padding, LSTM, resnet block, quantizer, chunking) is the parent's.  Pinned to the reference's own run by
``tests/test_encodec_gn_cpu.py`` over ``tests/golden/ref_encodec_gn_*.npz``."""
import math

import torch
import torch.nn.functional as F

from oracle.encodec_ref import EncodecRef


class EncodecGNRef(EncodecRef):
    def __init__(self, weights, config, dtype=torch.float32):
        cfg = dict(config)
        assert cfg.get("norm_type") == "time_group_norm"
        cfg["norm_type"] = "weight_norm"          # the parent's constructor only knows the plain convs; the norm is added below
        super().__init__(weights, cfg, dtype)
        self.c["norm_type"] = "time_group_norm"

    def group_norm(self, y, name):
        """y [B, L, C]: statistics in float64 whatever the working dtype (the fixture's GroupNorm does the same)."""
        d = y.double()
        mean = d.mean(dim=(1, 2), keepdim=True)
        var = d.var(dim=(1, 2), unbiased=False, keepdim=True)
        out = (d - mean) / torch.sqrt(var + 1e-5) * self.w[name + ".norm.weight"].double() + self.w[name + ".norm.bias"].double()
        return out.to(y.dtype)

    def conv(self, x, name, kernel_size, dilation=1, stride=1):
        return self.group_norm(super().conv(x, name, kernel_size, dilation=dilation, stride=stride), name)

    def convT(self, x, name, kernel_size, stride):
        c = self.c
        w = self.w[name + ".conv.weight"]  # [out, K, in]
        y = F.conv_transpose1d(x.transpose(1, 2), w.permute(2, 0, 1), self.w.get(name + ".conv.bias"), stride=stride).transpose(1, 2)
        y = self.group_norm(y, name)       # the FULL output, then the trim (encodec.py:275-291)
        padding_total = kernel_size - stride
        pr = math.ceil(padding_total * c["trim_right_ratio"]) if c["use_causal_conv"] else padding_total // 2
        pl = padding_total - pr
        return y[:, pl:y.shape[1] - pr]
