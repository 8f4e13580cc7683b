"""Plain-torch restatement of torchvision's ResNet-50 v1.5 and of the reference's ResNet wrapper (model.py:81-149):
the float64 yardstick of the HIP ResNet trunk. Written from the published architecture (He et al. 2016 with the
stride on the 3x3 conv, as torchvision ships it); module names and child order are torchvision's, so state_dict keys
match the reference checkpoints.
"""

import torch
from torch import nn

MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)


class Bottleneck(nn.Module):
    def __init__(self, inplanes, planes, stride=1, downsample=None):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.conv2 = nn.Conv2d(planes, planes, 3, stride=stride, padding=1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.conv3 = nn.Conv2d(planes, planes * 4, 1, bias=False)
        self.bn3 = nn.BatchNorm2d(planes * 4)
        self.relu = nn.ReLU()
        self.downsample = downsample
        self.stride = stride

    def forward(self, x):
        out = self.relu(self.bn1(self.conv1(x)))
        out = self.relu(self.bn2(self.conv2(out)))
        out = self.bn3(self.conv3(out))
        identity = self.downsample(x) if self.downsample is not None else x
        return self.relu(out + identity)


class ResNet50(nn.Module):
    def __init__(self, num_classes=1000):
        super().__init__()
        self.conv1 = nn.Conv2d(3, 64, 7, stride=2, padding=3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        self.relu = nn.ReLU()
        self.maxpool = nn.MaxPool2d(3, stride=2, padding=1)
        inplanes = 64
        for i, (planes, n, stride) in enumerate(((64, 3, 1), (128, 4, 2), (256, 6, 2), (512, 3, 2))):
            ds = nn.Sequential(nn.Conv2d(inplanes, planes * 4, 1, stride=stride, bias=False), nn.BatchNorm2d(planes * 4))
            blocks = [Bottleneck(inplanes, planes, stride, ds)] + [Bottleneck(planes * 4, planes) for _ in range(n - 1)]
            inplanes = planes * 4
            setattr(self, "layer%d" % (i + 1), nn.Sequential(*blocks))
        self.avgpool = nn.AdaptiveAvgPool2d(1)
        self.fc = nn.Linear(2048, num_classes)

    def forward(self, x):
        x = self.maxpool(self.relu(self.bn1(self.conv1(x))))
        x = self.layer4(self.layer3(self.layer2(self.layer1(x))))
        return self.fc(torch.flatten(self.avgpool(x), 1))


class Flatten(nn.Module):
    def forward(self, x):
        return torch.flatten(x, 1)


class CNN(nn.Module):
    """model.py:128-149 with the ResNet branch: frozen trunk, children[:-1] + flatten, or a new fc."""

    def __init__(self, just_bottlenecks=True, num_classes=10):
        super().__init__()
        self.cnn_model = ResNet50()
        for p in self.cnn_model.parameters():
            p.requires_grad = False
        if just_bottlenecks:
            self.cnn_model = nn.Sequential(*list(self.cnn_model.children())[:-1], Flatten())
        else:
            self.cnn_model.fc = nn.Linear(2048, num_classes)

    def forward(self, x):
        return self.cnn_model(x)


def normalize_input(x, conf):
    """model.py:84-101: (B, T, 1, 224, 224) -> (B*T, 3, 224, 224) normalised channels."""
    if conf == "repeat":
        x = torch.cat([x, x, x], dim=2)
    elif conf == "single":
        x = torch.cat([x, torch.zeros_like(x), torch.zeros_like(x)], dim=2)
    else:
        raise Exception("Invalid input type")
    x = x.clone()
    for c in range(3):
        x[:, :, c] = (x[:, :, c] - MEAN[c]) / STD[c]
    return x.reshape(-1, 3, 224, 224)
