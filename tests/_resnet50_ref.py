"""TEST INFRASTRUCTURE: torchvision's ResNet-50 (v1.5: stride on the 3x3 convolution) with fc = Identity, restated from nn.Conv2d / nn.BatchNorm2d /
F.max_pool2d / adaptive average pooling -- the oracle of maed_amd/resnet.py (torchvision itself is not a dependency of this project).  Module names are
torchvision's, so state dicts move between this restatement and the project's encoder with strict=True.  Tests run it in fp64."""
import torch
import torch.nn as nn
import torch.nn.functional as F


class RefBottleneck(nn.Module):
    def __init__(self, inplanes, planes, stride=1, downsample=None):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.conv2 = nn.Conv2d(planes, planes, 3, stride=stride, padding=1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.conv3 = nn.Conv2d(planes, planes * 4, 1, bias=False)
        self.bn3 = nn.BatchNorm2d(planes * 4)
        self.downsample = downsample

    def forward(self, x):
        out = F.relu(self.bn1(self.conv1(x)))
        out = F.relu(self.bn2(self.conv2(out)))
        out = self.bn3(self.conv3(out))
        identity = x if self.downsample is None else self.downsample(x)
        return F.relu(out + identity)


class RefResNet50(nn.Module):
    def __init__(self):
        super().__init__()
        self.conv1 = nn.Conv2d(3, 64, 7, stride=2, padding=3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        inplanes = 64
        for i, (planes, blocks, stride) in enumerate(((64, 3, 1), (128, 4, 2), (256, 6, 2), (512, 3, 2)), 1):
            down = nn.Sequential(nn.Conv2d(inplanes, planes * 4, 1, stride=stride, bias=False), nn.BatchNorm2d(planes * 4))
            layer = [RefBottleneck(inplanes, planes, stride, down)] + [RefBottleneck(planes * 4, planes) for _ in range(1, blocks)]
            inplanes = planes * 4
            setattr(self, f"layer{i}", nn.Sequential(*layer))
        self.fc = nn.Identity()

    def forward(self, x):
        x = F.max_pool2d(F.relu(self.bn1(self.conv1(x))), 3, 2, 1)
        x = self.layer4(self.layer3(self.layer2(self.layer1(x))))
        return self.fc(torch.flatten(F.adaptive_avg_pool2d(x, 1), 1))


def reference_of(encoder):
    """fp64 restatement carrying `encoder`'s parameters and buffers (loaded with strict=True), in the same train / eval mode"""
    ref = RefResNet50()
    ref.load_state_dict(encoder.state_dict(), strict=True)
    ref = ref.double()
    ref.train(encoder.training)
    return ref


def randomise(encoder, seed=0):
    """non-trivial BatchNorm parameters and buffers (a freshly initialised network has gamma = 1, beta = 0, running statistics 0 / 1).
    The last norm of every residual branch (bn3) gets a small gamma, 0.2 x the others: with gamma = 1 everywhere, sixteen un-trained blocks in train mode on the
    tests' tiny batches (16 values per channel in layer4) amplify fp32 rounding to the very bars the parity tests use -- the framework's own fp32 composition then
    sits at 0.4 .. 2.4 x the 1e-4 bar against fp64, whatever the seed.  Small branch gammas (torchvision's zero_init_residual starts them at 0, trained
    checkpoints keep them small) make the identity path dominate, and the same comparison sits at 0.01 .. 0.12 x the bar: the tests then measure the
    implementation, not the conditioning of a random network."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, t in encoder.state_dict().items():
            if name.endswith("bn3.weight"):
                t.copy_(((torch.rand(t.shape, generator=g) * 0.5 + 0.75) * 0.2).to(t.device))
            elif name.endswith("bn1.weight") or name.endswith("bn2.weight") or name.endswith("downsample.1.weight"):
                t.copy_((torch.rand(t.shape, generator=g) * 0.5 + 0.75).to(t.device))
            elif name.endswith(".bias"):
                t.copy_((torch.randn(t.shape, generator=g) * 0.1).to(t.device))
            elif name.endswith("running_mean"):
                t.copy_((torch.randn(t.shape, generator=g) * 0.1).to(t.device))
            elif name.endswith("running_var"):
                t.copy_((torch.rand(t.shape, generator=g) * 0.5 + 0.75).to(t.device))


def forward_with_decoder(ref, decoder, clip):
    """reference features (fp64) through the project's decoder: (features (N, T, 2048) fp64, the five outputs)"""
    N, T = clip.shape[:2]
    feat = ref(clip.double().reshape(N * T, *clip.shape[2:]))
    out = decoder(feat.float(), seqlen=T)
    out = dict(out)
    out["theta"] = out["theta"].reshape(N, T, -1)
    out["verts"] = out["verts"].reshape(N, T, -1, 3)
    out["kp_2d"] = out["kp_2d"].reshape(N, T, -1, 2)
    out["kp_3d"] = out["kp_3d"].reshape(N, T, -1, 3)
    out["rotmat"] = out["rotmat"].reshape(N, T, -1, 3, 3)
    return feat.reshape(N, T, -1), out


OUT_KEYS = ("theta", "verts", "kp_2d", "kp_3d", "rotmat")
LOSS_WTS = {"theta": 1.0, "kp_3d": 1.0, "kp_2d": 0.01}      # the loss of tests/test_gpu_model.py::test_maed_train_gradients_small_vs_oracle_f32


def loss_of(out):
    return sum(w * (out[k].double() ** 2).mean() for k, w in LOSS_WTS.items())
