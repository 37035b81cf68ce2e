"""The image encoder (the reference's models/encoder.py): a bottleneck ResNet from pixels to (fc [C], att [a, a, C]).

The module tree is written out here with torchvision's `ResNet` / `Bottleneck` parameter and buffer names (`conv1`,
`bn1`, `layer{1..4}.{i}.conv{1,2,3}`, `.bn{1,2,3}`, `.downsample.0`, `.downsample.1`, `fc`), so a `resnet101` checkpoint
loads with strict=True - torchvision itself is not needed.  As in the reference, the stride of layers 2-4 sits on
`conv1` of the first block (not on `conv2`) and the max-pool is 3x3 / 2, pad 0, ceil mode.

Native path (isc_encoder_fwd, csrc/encoder.hip) - ON by default whenever eligible: eval mode, tensors on the ROCm
device, fp32 parameters, no gradient asked for.  Every batch norm is folded into the convolution in front of it and the
weights are split into f16 planes once per weight version (repacked when a parameter's or buffer's `_version` or
`data_ptr` moves).  `enable_native(False)` runs the same network with stock torch ops: the A/B partner and the CPU path.
Forward only: no encoder training, no train-mode batch norm.
"""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib

MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)


class Bottleneck(nn.Module):
    expansion = 4

    def __init__(self, inplanes, planes, stride=1, downsample=None):
        super().__init__()
        # (the reference moves the stride from conv2 to conv1: encoder.py:13-15)
        self.conv1 = nn.Conv2d(inplanes, planes, 1, stride=stride, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.conv2 = nn.Conv2d(planes, planes, 3, stride=1, padding=1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.conv3 = nn.Conv2d(planes, planes * 4, 1, bias=False)
        self.bn3 = nn.BatchNorm2d(planes * 4)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = downsample

    def forward(self, x):
        out = self.relu(self.bn1(self.conv1(x)))
        out = self.relu(self.bn2(self.conv2(out)))
        out = self.bn3(self.conv3(out))
        identity = x if self.downsample is None else self.downsample(x)
        return self.relu(out + identity)


class ResNet(nn.Module):
    """torchvision's ResNet over Bottleneck blocks (its names), with the reference's two changes."""

    def __init__(self, layers=(3, 4, 23, 3), width=64, num_classes=1000):
        super().__init__()
        self.layers, self.width = tuple(int(n) for n in layers), int(width)
        assert len(self.layers) == 4 and all(n >= 1 for n in self.layers)
        self.inplanes = self.width
        self.conv1 = nn.Conv2d(3, self.width, 7, stride=2, padding=3, bias=False)
        self.bn1 = nn.BatchNorm2d(self.width)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(kernel_size=3, stride=2, padding=0, ceil_mode=True)
        for l, n in enumerate(self.layers):
            setattr(self, 'layer%d' % (l + 1), self._make_layer(self.width << l, n, 1 if l == 0 else 2))
        self.avgpool = nn.AdaptiveAvgPool2d((1, 1))
        self.fc = nn.Linear(self.width * 32, num_classes)     # (unused by the encoder; part of the checkpoint)

    def _make_layer(self, planes, blocks, stride):
        downsample = nn.Sequential(nn.Conv2d(self.inplanes, planes * 4, 1, stride=stride, bias=False),
                                   nn.BatchNorm2d(planes * 4))
        seq = [Bottleneck(self.inplanes, planes, stride, downsample)]
        self.inplanes = planes * 4
        seq += [Bottleneck(self.inplanes, planes) for _ in range(1, blocks)]
        return nn.Sequential(*seq)

    def features(self, x):
        x = self.maxpool(self.relu(self.bn1(self.conv1(x))))
        return self.layer4(self.layer3(self.layer2(self.layer1(x))))

    def conv_bn_pairs(self):
        """[(conv, bn)] in the library's order: the stem, then per block conv1, conv2, conv3 and the downsample."""
        out = [(self.conv1, self.bn1)]
        for l in range(4):
            for blk in getattr(self, 'layer%d' % (l + 1)):
                out += [(blk.conv1, blk.bn1), (blk.conv2, blk.bn2), (blk.conv3, blk.bn3)]
                if blk.downsample is not None:
                    out.append((blk.downsample[0], blk.downsample[1]))
        return out


class Encoder(nn.Module):
    native = True

    def __init__(self, resnet101_file=None, layers=(3, 4, 23, 3), width=64):
        super().__init__()
        resnet = ResNet(layers, width)
        if resnet101_file is not None:
            resnet.load_state_dict(torch.load(resnet101_file, map_location=lambda s, l: s), strict=True)
        self.resnet = resnet
        for p in resnet.parameters():       # frozen, as the reference uses it (under no_grad, in eval mode)
            p.requires_grad_(False)
        self.native = True
        self._native_pack = None        # (key, packed): rebuilt when a tensor's (data_ptr, _version) moves

    # ---- native switch
    def enable_native(self, on=True):
        self.native = bool(on)
        return self

    def native_tensors(self):
        out = []
        for conv, bn in self.resnet.conv_bn_pairs():
            out.append((conv.weight, bn.weight, bn.bias, bn.running_mean, bn.running_var))
        return out

    def native_active(self, image):
        """Whether a forward takes the native path now: the flag is on, eval mode, the image and the fp32 parameters live
        on the same ROCm device and nothing asks for a gradient.  Everything else runs the torch ops."""
        w = self.resnet.conv1.weight
        if not self.native or self.training or not torch.is_tensor(image) or not image.is_cuda:
            return False
        if w.device != image.device or w.dtype != torch.float32:
            return False
        return not (torch.is_grad_enabled() and any(p.requires_grad for p in self.resnet.parameters()))

    def packed(self):
        from . import ops
        tensors = self.native_tensors()
        key = tuple((t.data_ptr(), t._version) for c in tensors for t in c)
        if self._native_pack is None or self._native_pack[0] != key:
            with torch.no_grad():
                convs = [tuple(t.detach().contiguous() for t in c) for c in tensors]
                self._native_pack = (key, ops.encoder_pack(convs, self.resnet.layers, self.resnet.width))
        return self._native_pack[1]

    # ---- the reference's surface
    def preprocess(self, image):
        """uint8 (or any numeric) array [H, W] or [H, W, 3] -> normalised fp32 tensor [3, H, W] (encoder.py:29-37)."""
        image = np.asarray(image)
        if image.ndim == 2:
            image = image[:, :, np.newaxis]
            image = np.concatenate((image, image, image), axis=2)
        image = image.astype('float32') / 255.0
        image = torch.from_numpy(np.ascontiguousarray(image.transpose(2, 0, 1)))
        mean = torch.tensor(MEAN, dtype=torch.float32).view(3, 1, 1)
        std = torch.tensor(STD, dtype=torch.float32).view(3, 1, 1)
        return (image - mean) / std

    def _torch_batch(self, x, att_size):
        """x [B, 3, H, W] normalised -> (fc [B, C], att [B, a, a, C]) with stock torch ops."""
        x = self.resnet.features(x)
        fc = x.mean(3).mean(2)
        att = F.adaptive_avg_pool2d(x, [att_size, att_size]).permute(0, 2, 3, 1)
        return fc, att.contiguous()

    def _native_batch(self, hwc, att_size, ksplit=0, want_f16=False):
        from . import ops
        with torch.no_grad():
            return ops.encoder_fwd(self.packed(), hwc, self.resnet.layers, self.resnet.width, att_size, ksplit=ksplit,
                                   want_f16=want_f16)

    def forward_batch(self, imgs, att_size=14, want_f16=False):
        """imgs [B, 3, H, W] normalised fp32 (B equal-sized `preprocess` outputs) -> (fc [B, C], att [B, a, a, C]);
        want_f16: also their float16 copies (what the float16 feature stores hold)."""
        if self.native_active(imgs):
            return self._native_batch(imgs.permute(0, 2, 3, 1).contiguous().float(), att_size, want_f16=want_f16)
        fc, att = self._torch_batch(imgs, att_size)
        return (fc, att, fc.half(), att.half()) if want_f16 else (fc, att)

    def forward(self, img, att_size=14):
        """img [3, H, W] (`preprocess`) -> (fc [C], att [a, a, C]) (encoder.py:39-55; the reference's squeeze() would
        also drop a 1-sized grid or att_size dimension - here the shapes are always these)."""
        fc, att = self.forward_batch(img.unsqueeze(0), att_size)
        return fc[0], att[0]

    def encode_uint8(self, img_hwc, att_size=14, want_f16=False):
        """img_hwc: uint8 [H, W, 3] or [B, H, W, 3] as decoded (tensor or array; grey [H, W] is repeated) -> forward /
        forward_batch of its `preprocess`; on the native path the normalisation is fused into the stem's loads."""
        t = img_hwc if torch.is_tensor(img_hwc) else torch.from_numpy(np.array(img_hwc))
        assert t.dtype == torch.uint8, 'encode_uint8 takes uint8 pixels'
        if t.dim() == 2:
            t = t.unsqueeze(-1).expand(-1, -1, 3)
        single = t.dim() == 3
        if single:
            t = t.unsqueeze(0)
        t = t[..., :3]
        dev = self.resnet.conv1.weight.device
        t = t.to(dev)
        if self.native_active(t):
            out = self._native_batch(t.contiguous(), att_size, want_f16=want_f16)
        else:
            x = t.float() / 255.0
            mean = torch.tensor(MEAN, dtype=torch.float32, device=dev)
            std = torch.tensor(STD, dtype=torch.float32, device=dev)
            out = self.forward_batch(((x - mean) / std).permute(0, 3, 1, 2).contiguous(), att_size, want_f16=want_f16)
        return tuple(o[0] for o in out) if single else out
