"""Stage-1 encoder: torchvision-layout ResNet-50 with BatchNorm (reference: lib/models/maed.py:35-37 -- `torchvision.models.resnet50` with fc = Identity,
the encoder of MAED(encoder='cnn'), configs/config_stage1.yaml).

Module tree and parameter names are torchvision's (conv1, bn1, layer1..4 of (3, 4, 6, 3) bottlenecks with the stride on the 3x3 conv2, downsample.0 / .1,
avgpool, fc), so a torchvision or stage-1 checkpoint loads with strict=True.  What this module decides is the MI355X side: activations are channels_last in
the compute dtype; BatchNorm (+ residual add + ReLU), the 3x3/2 max-pool and the global average pool are libmaed_hip streaming kernels (csrc/batchnorm.hip);
the convolutions are the library's GEMM / implicit-GEMM / stem kernels the GroupNorm backbone (resnetv2.py) already uses, fed with plain -- unstandardised --
weight images (ops.WeightImageFn); a shape outside a kernel's precondition takes the framework's convolution.

The norm layer is NOT a torch.nn.modules.batchnorm._BatchNorm: torch.nn.SyncBatchNorm.convert_sync_batchnorm (reference train.py:95) leaves it in place.
Statistics over the batch of all ranks are opt-in: convert_sync_batchnorm below (docs/design/16_sync_batchnorm.md); without it every rank normalises with its
own batch.
"""
import os
from collections import OrderedDict

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops

# A/B knob: MAED_CNN_BN=torch puts BatchNorm, max-pool and average pool on the framework's composition (host side, like the MAED_*=0 switches of resnetv2.py)
_LIB_BN = os.environ.get("MAED_CNN_BN", "own") != "torch"


def _slots(module, **values):
    module.__dict__.update(values)       # per-pass hand-over slots: plain attributes, past nn.Module.__setattr__ (resnetv2._slots)


def bn_qualifies(C_, rows, dtype):
    """host-side predicate of the library BatchNorm / pools: channels_last rows of C % 8 == 0 channels in fp32 or bf16, fewer than 2^31 rows"""
    return C_ % 8 == 0 and 0 < rows < 1 << 31 and dtype in (torch.float32, torch.bfloat16)


def conv_route(kernel, stride, cin, cout, rows_out, dtype, prec=None):
    """which kernel a convolution of this encoder runs on -- 'gemm' (ops.Conv1x1Fn), 'conv3x3' (ops.Conv3x3Fn: stride 1, where TF-SAME is padding 1),
    'conv3x3s2' (ops.Conv3x3S2P1Fn) -- or 'aten': the framework's convolution, for a dtype without library matrix products (fp32 on the exact engine) or a shape
    outside the kernels' preconditions (channel counts that are no multiple of 64, a row count that is no multiple of the 64-row tile).  The stem is decided by
    ResNet.plan (it depends on the frame geometry: ops.stem7x7s2_supported)."""
    if not ops.lib_matmul_dtype(dtype, prec) or cin % 64 or cout % 64 or rows_out % 64 or rows_out <= 0:
        return "aten"
    if kernel == 1 and stride in (1, 2):
        return "gemm"
    if kernel == 3:
        return "conv3x3" if stride == 1 else "conv3x3s2" if stride == 2 else "aten"
    return "aten"


class Conv2d(nn.Conv2d):
    """zero-padded symmetric convolution without bias; inside ResNet.forward the slots below carry this pass's weight image and route"""
    _w = None       # compute-dtype image, logical (O, I, kh, kw) over (O, kh, kw, I) storage (ops.WeightImageFn)
    _wt = None      # transposed image (kh*kw*I, O)
    _dw = None      # fp32 (O, kh*kw*I) slice the weight gradient accumulates into
    _route = "aten"
    _prec = None
    _stem_hw = None

    def forward(self, x):
        w = self._w
        if w is None:                       # stand-alone use / CPU
            return F.conv2d(x, self.weight.to(x.dtype), None, self.stride, self.padding)
        r = self._route
        if r == "gemm":
            return ops.Conv1x1Fn.apply(x, w, self._wt, self._dw, False, None, self.stride[0], False, self._prec)
        if r == "conv3x3":
            return ops.Conv3x3Fn.apply(x, w, 1, self._wt, self._dw, None, self._prec)
        if r == "conv3x3s2":
            return ops.Conv3x3S2P1Fn.apply(x, w, self._wt, self._dw, self._prec)
        if r == "stem":                     # x: the padded 4-slot image of ops.stem_input_pad3
            return ops.StemConvFn.apply(x, w, self._dw, None, self._stem_hw)
        return F.conv2d(x, w, None, self.stride, self.padding)


class BatchNorm2d(nn.Module):
    """nn.BatchNorm2d's parameters, buffers and arithmetic (eps inside the root, biased batch variance for normalising, unbiased for running_var), with the
    residual add and the ReLU of a bottleneck fused in: forward(x, residual=None, relu=False) = act(BN(x) [+ residual])."""

    def __init__(self, num_features, eps=1e-5, momentum=0.1):
        super().__init__()
        self.num_features, self.eps, self.momentum = num_features, eps, momentum
        self.weight = nn.Parameter(torch.ones(num_features))
        self.bias = nn.Parameter(torch.zeros(num_features))
        self.register_buffer("running_mean", torch.zeros(num_features))
        self.register_buffer("running_var", torch.ones(num_features))
        self.register_buffer("num_batches_tracked", torch.tensor(0, dtype=torch.long))
        self.sync = None        # ops.StatSync (convert_sync_batchnorm): training statistics over the batch of all ranks

    def extra_repr(self):
        return f"{self.num_features}, eps={self.eps}, momentum={self.momentum}"

    def forward(self, x, residual=None, relu=False):
        rows = x.numel() // x.shape[1]
        sync = self.sync if (self.training and self.sync is not None and self.sync.active) else None
        if self.training and rows <= 1 and (sync is None or sync.world == 1):
            raise ValueError(f"Expected more than 1 value per channel when training, got input size {tuple(x.shape)}")
        if sync is not None and rows < 1:
            raise ValueError(f"statistics over all ranks need at least one row on every rank, got input size {tuple(x.shape)}")
        if _LIB_BN and ops.on_library_device(x) and bn_qualifies(x.shape[1], rows, x.dtype):
            if self.training:
                self.num_batches_tracked.add_(1)
            return ops.BatchNormFn.apply(x, residual, self.weight, self.bias, (self.running_mean, self.running_var), self.training, self.momentum, self.eps, relu, sync)
        if self.training:
            self.num_batches_tracked.add_(1)
        if sync is not None:
            y = ops.SyncBatchNormTorchFn.apply(x, self.weight, self.bias, self.running_mean, self.running_var, self.momentum, self.eps, sync)
        else:
            y = F.batch_norm(x, self.running_mean, self.running_var, self.weight, self.bias, self.training, self.momentum, self.eps)
        if residual is not None:
            y = y + residual
        return F.relu(y) if relu else y


def convert_sync_batchnorm(module, process_group=None, comm=None, force_collectives=False):
    """torch.nn.SyncBatchNorm.convert_sync_batchnorm (reference train.py:95) for this module's norm layers: every BatchNorm2d under `module` takes its training
    statistics over the batch of all ranks of `process_group` (torch.distributed; None = the default group) or of `comm` (a ddp.RcclComm).  The modules stay in
    place (state-dict keys do not change); one reducer is shared by all of them.  No collective is issued in eval mode or in a world of one, unless
    force_collectives asks for them there.  The stat collectives and the gradient buckets share a communicator: every rank must issue both kinds from one host
    thread, in program order (docs/design/16_sync_batchnorm.md).  Returns `module`."""
    sync = ops.StatSync(process_group, comm, force_collectives)
    for m in module.modules():
        if isinstance(m, BatchNorm2d):
            m.sync = sync
    return module


class MaxPool3s2P1(nn.Module):
    """nn.MaxPool2d(kernel_size=3, stride=2, padding=1)"""

    def forward(self, x):
        if _LIB_BN and ops.on_library_device(x) and bn_qualifies(x.shape[1], x.numel() // x.shape[1], x.dtype):
            return ops.MaxPool3s2P1Fn.apply(x)
        return F.max_pool2d(x, 3, 2, 1)


class GlobalAvgPool(nn.Module):
    """nn.AdaptiveAvgPool2d(1) + flatten: (F, C, H, W) -> (F, C); fp32 on the library"""

    def forward(self, x):
        if _LIB_BN and ops.on_library_device(x) and bn_qualifies(x.shape[1], x.numel() // x.shape[1], x.dtype):
            return ops.GlobalAvgPoolFn.apply(x)
        return F.adaptive_avg_pool2d(x, 1).flatten(1)


class Bottleneck(nn.Module):
    expansion = 4

    def __init__(self, inplanes, planes, stride=1, downsample=None):
        super().__init__()
        self.conv1 = Conv2d(inplanes, planes, 1, bias=False)
        self.bn1 = BatchNorm2d(planes)
        self.conv2 = Conv2d(planes, planes, 3, stride=stride, padding=1, bias=False)       # torchvision: the stride sits on the 3x3 (ResNet v1.5)
        self.bn2 = BatchNorm2d(planes)
        self.conv3 = Conv2d(planes, planes * self.expansion, 1, bias=False)
        self.bn3 = BatchNorm2d(planes * self.expansion)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = downsample
        self.stride = stride

    def forward(self, x):
        out = self.bn1(self.conv1(x), relu=True)
        out = self.bn2(self.conv2(out), relu=True)
        out = self.conv3(out)
        identity = x if self.downsample is None else self.downsample(x)
        return self.bn3(out, residual=identity, relu=True)         # BN + shortcut add + ReLU in one pass


class ResNet(nn.Module):
    def __init__(self, layers=(3, 4, 6, 3), compute_dtype=torch.float32, f32_matmul=None):
        super().__init__()
        assert f32_matmul in (None, "bf16x3", "bf16x6"), f32_matmul
        self.compute_dtype, self.f32_matmul = compute_dtype, f32_matmul
        self.inplanes = 64
        self.conv1 = Conv2d(3, 64, 7, stride=2, padding=3, bias=False)
        self.bn1 = BatchNorm2d(64)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = MaxPool3s2P1()
        self.layer1 = self._make_layer(64, layers[0], 1)
        self.layer2 = self._make_layer(128, layers[1], 2)
        self.layer3 = self._make_layer(256, layers[2], 2)
        self.layer4 = self._make_layer(512, layers[3], 2)
        self.avgpool = GlobalAvgPool()
        self.fc = nn.Identity()                                     # maed.py:36
        self.num_features = 512 * Bottleneck.expansion
        for m in self.modules():                                    # torchvision's initialisation
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")
        self._convs = [m for m in self.modules() if isinstance(m, Conv2d)]
        self._norms = [m for m in self.modules() if isinstance(m, BatchNorm2d)]
        self._direct_convs = []
        self._w_t, self._dw_slices = {}, {}

    def _make_layer(self, planes, blocks, stride):
        downsample = None
        if stride != 1 or self.inplanes != planes * Bottleneck.expansion:
            downsample = nn.Sequential(Conv2d(self.inplanes, planes * Bottleneck.expansion, 1, stride=stride, bias=False), BatchNorm2d(planes * Bottleneck.expansion))
        layers = [Bottleneck(self.inplanes, planes, stride, downsample)]
        self.inplanes = planes * Bottleneck.expansion
        layers += [Bottleneck(self.inplanes, planes) for _ in range(1, blocks)]
        return nn.Sequential(*layers)

    def conv_weights(self):
        return [c.weight for c in self._convs]

    def plan(self, F_, H, W, dtype=None, stem_fused=True):
        """host-side kernel selection for F_ frames of H x W: {'convs': [(name, route)] in self._convs order, 'norms': [(name, bool)], 'pools': [(name, bool)]}"""
        dtype = self.compute_dtype if dtype is None else dtype
        names = {id(m): n for n, m in self.named_modules()}
        geo = {}                                                    # id(conv) -> (rows_out), walked in forward order

        def out_hw(h, w, k, s, p):
            return (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1

        h, w = out_hw(H, W, 7, 2, 3)
        stem_ok = (stem_fused and dtype == torch.bfloat16 and os.environ.get("MAED_STEM_OWN", "1") == "1" and H % 2 == 0 and W % 2 == 0
                   and ops.stem7x7s2_supported(H, W, F_))
        norms, pools = [(names[id(self.bn1)], bn_qualifies(64, F_ * h * w, dtype))], [("maxpool", bn_qualifies(64, F_ * h * w, dtype))]
        routes = {id(self.conv1): "stem" if stem_ok else "aten"}
        h, w = out_hw(h, w, 3, 2, 1)
        for layer in (self.layer1, self.layer2, self.layer3, self.layer4):
            for blk in layer:
                s = blk.stride
                ho, wo = out_hw(h, w, 3, s, 1)
                for conv, bn, rows in ((blk.conv1, blk.bn1, F_ * h * w), (blk.conv2, blk.bn2, F_ * ho * wo), (blk.conv3, blk.bn3, F_ * ho * wo)):
                    routes[id(conv)] = conv_route(conv.kernel_size[0], conv.stride[0], conv.in_channels, conv.out_channels, rows, dtype, self.f32_matmul)
                    norms.append((names[id(bn)], bn_qualifies(conv.out_channels, rows, dtype)))
                if blk.downsample is not None:
                    conv, bn = blk.downsample[0], blk.downsample[1]
                    routes[id(conv)] = conv_route(1, conv.stride[0], conv.in_channels, conv.out_channels, F_ * ho * wo, dtype, self.f32_matmul)
                    norms.append((names[id(bn)], bn_qualifies(conv.out_channels, F_ * ho * wo, dtype)))
                h, w = ho, wo
        pools.append(("avgpool", bn_qualifies(self.num_features, F_ * h * w, dtype)))
        return {"convs": [(names[id(c)], routes[id(c)]) for c in self._convs], "norms": norms, "pools": pools}

    def _forward_plain(self, x):
        x = self.maxpool(self.bn1(self.conv1(x), relu=True))
        x = self.layer4(self.layer3(self.layer2(self.layer1(x))))
        return self.fc(self.avgpool(x))

    def forward(self, x, seqlen=None):
        if not ops.on_library_device(x):
            return self._forward_plain(x)
        try:
            return self._forward_library(x)
        finally:
            for c in self._convs:
                _slots(c, _w=None, _wt=None, _dw=None, _route="aten", _prec=None, _stem_hw=None)

    def _forward_library(self, x):
        cdt = self.compute_dtype
        F_, _, H, W = x.shape
        stem_fused = x.dtype == torch.float32 and x.is_contiguous() and x.shape[1] == 3 and not x.requires_grad
        routes = [r for _, r in self.plan(F_, H, W, cdt, stem_fused)["convs"]]
        self._direct_convs = [i for i, r in enumerate(routes) if r != "aten"]
        ws = ops.WeightImageFn.apply(self, cdt, *self.conv_weights())
        for i, (c, w, r) in enumerate(zip(self._convs, ws, routes)):
            _slots(c, _w=w, _wt=self._w_t.get(i), _dw=self._dw_slices.get(i), _route=r, _prec=self.f32_matmul)
        if routes[0] == "stem":
            _slots(self.conv1, _stem_hw=(H, W))
            x = ops.stem_input_pad3(x, cdt)
        else:
            x = x.to(dtype=cdt, memory_format=torch.channels_last)
        return self._forward_plain(x)


def resnet50(pretrained=False, compute_dtype=torch.float32, f32_matmul=None, **_):
    """torchvision.models.resnet50 with fc = Identity (maed.py:35-36).  `pretrained` downloads nothing here: load the torchvision / stage-1 state_dict yourself
    with load_state_dict(strict=True)."""
    if pretrained:
        raise NotImplementedError("pretrained=True needs network access; load the checkpoint with load_state_dict")
    return ResNet((3, 4, 6, 3), compute_dtype=compute_dtype, f32_matmul=f32_matmul)
