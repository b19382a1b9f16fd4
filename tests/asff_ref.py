"""Plain-PyTorch restatement of the reference's ASFF head, the CPU oracle of tests/test_asff_host.py and tests/test_asff_gpu.py:
add_conv (models/common.py:5322-5343: Conv2d(bias=False) -> BatchNorm2d -> LeakyReLU(0.1), children `conv` / `batch_norm` / `leaky`), ASFF
(models/common.py:5500-5567) and ASFF_Detect (models/yolo.py:172-184), written from their semantics:

  * ASFF(level) brings P5 / P4 / P3 (512 / 256 / 128 channels) to the level's width and size - 3x3 stride-2 conv one level down,
    max_pool2d(3, 2, 1) + 3x3 stride-2 conv two levels down, 1x1 conv + nearest upsampling up -, makes a 16-channel map of each, turns their concat
    into three logits per pixel with a 48 -> 3 1x1 conv (with bias), and sends the softmax-weighted sum through a 3x3 `expand` conv;
  * ASFF_Detect rewrites its reversed input list in place while it walks it: f0 = asff0(P5, P4, P3), f1 = asff1(f0, P4, P3),
    f2 = asff2(f0, f1, P3), Detect on [f2, f1, f0].  tests/golden/block_asff*.npz, generated from the reference's own classes, pin that.

oracle_model(cfg) builds the oracle Model of a cfg whose head row names ASFF_Detect; Packed3 / PackedHead are one-tensor shells that let
parity.check_block drive these three-input blocks."""
import copy

import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle.somi_ref import blocks as OB


def add_conv(in_ch, out_ch, ksize, stride, leaky=True):
    stage = nn.Sequential()
    stage.add_module('conv', nn.Conv2d(in_ch, out_ch, ksize, stride, (ksize - 1) // 2, bias=False))
    stage.add_module('batch_norm', nn.BatchNorm2d(out_ch))
    stage.add_module('leaky', nn.LeakyReLU(0.1) if leaky else nn.ReLU6(inplace=True))
    return stage


class ASFF(nn.Module):
    def __init__(self, level, rfb=False, vis=False):
        super().__init__()
        self.level = level
        self.dim = [512, 256, 128]
        self.inter_dim = c = self.dim[level]
        if level == 0:
            self.stride_level_1 = add_conv(256, c, 3, 2)
            self.stride_level_2 = add_conv(128, c, 3, 2)
            self.expand = add_conv(c, 512, 3, 1)
        elif level == 1:
            self.compress_level_0 = add_conv(512, c, 1, 1)
            self.stride_level_2 = add_conv(128, c, 3, 2)
            self.expand = add_conv(c, 256, 3, 1)
        else:
            self.compress_level_0 = add_conv(512, c, 1, 1)
            self.compress_level_1 = add_conv(256, c, 1, 1)
            self.expand = add_conv(c, 128, 3, 1)
        compress_c = 8 if rfb else 16
        self.weight_level_0 = add_conv(c, compress_c, 1, 1)
        self.weight_level_1 = add_conv(c, compress_c, 1, 1)
        self.weight_level_2 = add_conv(c, compress_c, 1, 1)
        self.weight_levels = nn.Conv2d(compress_c * 3, 3, 1)
        self.vis = vis

    def forward(self, x0, x1, x2):
        if self.level == 0:
            r0, r1 = x0, self.stride_level_1(x1)
            r2 = self.stride_level_2(F.max_pool2d(x2, 3, stride=2, padding=1))
        elif self.level == 1:
            r0 = F.interpolate(self.compress_level_0(x0), scale_factor=2, mode='nearest')
            r1, r2 = x1, self.stride_level_2(x2)
        else:
            r0 = F.interpolate(self.compress_level_0(x0), scale_factor=4, mode='nearest')
            r1 = F.interpolate(self.compress_level_1(x1), scale_factor=2, mode='nearest')
            r2 = x2
        v = torch.cat((self.weight_level_0(r0), self.weight_level_1(r1), self.weight_level_2(r2)), 1)
        p = F.softmax(self.weight_levels(v), dim=1)
        return self.expand(r0 * p[:, 0:1] + r1 * p[:, 1:2] + r2 * p[:, 2:])


class ASFF_Detect(OB.Detect):
    def __init__(self, nc=80, anchors=(), ch=(), inplace=False):
        super().__init__(nc, anchors, ch, inplace)
        self.asffs = nn.ModuleList(ASFF(i) for i in range(self.nl))

    def forward(self, x):
        x = list(x)[::-1]
        for i in range(self.nl):
            x[i] = self.asffs[i](*x)                              # in place: the later levels see the fused coarser maps
        return super().forward(x[::-1])


def oracle_model(cfg):
    """The oracle Model of `cfg` (head row ASFF_Detect): built with a Detect row - ASFF changes no map size, so strides, scaled and ordered
    anchors and the bias init are Detect's -, then the last layer is swapped for the restated head around the same 1x1 convs."""
    from oracle.somi_ref import Model as OModel
    assert cfg['head'][-1][2] == 'ASFF_Detect'
    plain = copy.deepcopy(cfg)
    plain['head'][-1][2] = 'Detect'
    model = OModel(plain)
    old = model.model[-1]
    head = ASFF_Detect(old.nc, [[0.0] * (2 * old.na)] * old.nl, [m.in_channels for m in old.m], old.inplace)
    head.anchors.copy_(old.anchors)
    head.m, head.stride = old.m, old.stride
    head.i, head.f, head.type = old.i, old.f, 'ASFF_Detect'
    head.np = sum(p.numel() for p in head.parameters())
    model.model[-1] = head
    model.yaml = copy.deepcopy(cfg)
    OB.initialize_weights(model)
    return model


# ---------------------------------------------------------------------------------------------- the graph case
# fill_state seed and synthetic_batch seed of the graph test (yolov5s + ASFF_Detect, nc 10, batch 2, 96x64).  LeakyReLU has a kink, the head holds
# 130 000 of its inputs at this size, and a training forward in fp32 sits 1e-4 .. 2e-4 from its fp64 twin behind the batch-statistics BatchNorms
# (12 pixels per channel at P5): wherever one pre-activation lies closer to zero than that, two correct fp32 forwards can take different sides, and
# one flipped element moves its layer's BatchNorm bias gradient by tens of check_train_step's bars (2e-3 * scale + 2e-6) and everything upstream by
# several.  The fp32 CPU oracle against its OWN fp64 twin, worst parameter gradient in bars: seeds (3, 2), the pair the Swin graph test uses: 11.5
# (197 parameters beyond the bar, one flipped element in asffs.1.expand); (4, 2): 77; (1, 0): 12.8; (3, 3): 6.0; with SiLU in LeakyReLU's place
# (3, 2) gives 0.24, and the plain-Detect graph 0.03.  (5, 7) leaves the oracle at 0.09 from fp64, yet the MI355X path flipped one element of
# asffs.0.stride_level_1 there (that layer's BatchNorm bias 31 bars off, every other head parameter below 0.1).  So the pair is chosen from the
# reference alone, by the margin that matters: of the 24 pairs (1..6) x (0..3), the one whose fp64 oracle keeps every LeakyReLU input of the head
# farthest from zero - (5, 2), 4.6e-5 (the others: 2e-6 .. 2.5e-5) - and tests/test_asff_host.py asserts that the fp32 oracle is within a quarter
# of the bar of fp64 there.
GRAPH_SEEDS = (5, 2)


def graph_case():
    """-> (cfg, the filled oracle model, images, targets) of the graph test."""
    from oracle.somi_ref.testing import HYP_VISDRONE, fill_state, synthetic_batch
    from somi_amd.configs import yolov5_cfg
    cfg = yolov5_cfg(0.5, 0.33, nc=10, head='ASFF_Detect')
    ref = fill_state(oracle_model(cfg), GRAPH_SEEDS[0])
    ref.hyp = dict(HYP_VISDRONE)
    imgs, targets = synthetic_batch(2, 96, nc=10, seed=GRAPH_SEEDS[1])
    return cfg, ref, imgs[..., :64].contiguous(), targets


# ---------------------------------------------------------------------------------------------- one-tensor shells for parity.check_block
# The three maps of a pyramid travel as ONE tensor at P5's size: P5's 512 channels, then P4 (256 channels, 2x the size) and P3 (128 channels,
# 4x) folded into 1024 and 2048 channels the way F.pixel_unshuffle does (channel c * r * r + dy * r + dx = pixel (h * r + dy, w * r + dx)).
PACKED = 512 + 1024 + 2048
STRIDES = (8.0, 16.0, 32.0)
ANCHORS = [[1.25, 1.625, 2.0, 3.75, 4.125, 2.875], [1.875, 3.8125, 3.875, 2.8125, 3.6875, 7.4375], [3.625, 2.8125, 4.875, 6.1875, 11.65625, 10.1875]]


def unpack_nchw(x):
    return x[:, :512], F.pixel_shuffle(x[:, 512:1536], 2), F.pixel_shuffle(x[:, 1536:], 4)


def _unfold_nhwc(t, c, r):
    B, h, w, _ = t.shape
    return t.reshape(B, h, w, c, r, r).permute(0, 1, 4, 2, 5, 3).reshape(B, h * r, w * r, c).contiguous()


def _fold_nhwc(t, r):
    B, H, W, c = t.shape
    return t.reshape(B, H // r, r, W // r, r, c).permute(0, 1, 3, 5, 2, 4).reshape(B, H // r, W // r, c * r * r)


class _Shell(nn.Module):
    def __init__(self, ns, build):
        super().__init__()
        self.m = build(ns)
        self.native = hasattr(ns, 'Act')                          # somi_amd.blocks: Acts in, Acts out

    def _acts(self, a):
        Act = type(a)
        t = a.t[..., a.coff:a.coff + PACKED]
        return [Act(t[..., :512].contiguous()), Act(_unfold_nhwc(t[..., 512:1536], 256, 2)), Act(_unfold_nhwc(t[..., 1536:], 128, 4))]

    @staticmethod
    def _pack_grads(Act, d0, d1, d2):
        chan = lambda d, c: d.t[..., d.coff:d.coff + c]           # noqa: E731
        return Act(torch.cat([chan(d0, 512), _fold_nhwc(chan(d1, 256), 2), _fold_nhwc(chan(d2, 128), 4)], -1).contiguous())


class Packed3(_Shell):
    """ASFF(level) behind one packed input."""

    def forward(self, x):
        return self.m(*self._acts(x)) if self.native else self.m(*unpack_nchw(x))

    def backward(self, dout):
        return self._pack_grads(type(dout), *self.m.backward(dout))


class PackedHead(_Shell):
    """ASFF_Detect behind one packed input; the training outputs (or, in eval, z and the raws) come back flattened into one (B, N, 1, 1) map."""

    def __init__(self, ns, build):
        super().__init__(ns, build)
        self.m.stride = torch.tensor(STRIDES)

    def forward(self, x):
        if self.native:
            p5, p4, p3 = self._acts(x)
            out = self.m([p3, p4, p5])
        else:
            p5, p4, p3 = unpack_nchw(x)
            out = self.m([p3, p4, p5])
        raws = out if self.training else [out[0]] + list(out[1])
        self.__dict__['_shapes'] = [tuple(r.shape) for r in raws]
        flat = torch.cat([r.reshape(r.shape[0], -1) for r in raws], 1)
        if self.native:
            return type(x)(flat.reshape(flat.shape[0], 1, 1, -1).contiguous())
        return flat.reshape(flat.shape[0], -1, 1, 1)

    def backward(self, dout):
        flat, draws, o = dout.t.reshape(dout.t.shape[0], -1), [], 0
        for s in self._shapes:
            n = s[1] * s[2] * s[3] * s[4]
            draws.append(flat[:, o:o + n].reshape(s).contiguous())
            o += n
        dp3, dp4, dp5 = self.m.backward(draws)
        return self._pack_grads(type(dout), dp5, dp4, dp3)
