"""Float64 restatement of torchvision's Inception3 feature path (eval mode, transform_input=False, fc = Identity) in
torch.nn.functional, NCHW, torchvision key names: the truth the device extractor is tested against.  It restates the
network from torchvision's module definitions (kernel sizes, strides, paddings written out below), not from the
package's own table.  Also: random weights with BatchNorm statistics calibrated on this network."""
import torch
import torch.nn.functional as F

MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)
EPS = 1e-3


def preprocess(images, in_scale, in_shift):
    """[N, 3, 299, 299]: in_scale * x + in_shift, transforms.Resize((299, 299)) (bilinear, half-pixel), Normalize."""
    x = images.to(torch.float64) * in_scale + in_shift
    x = F.interpolate(x, size=(299, 299), mode="bilinear", align_corners=False)
    mean = torch.tensor(MEAN, dtype=torch.float64, device=x.device).view(1, 3, 1, 1)
    std = torch.tensor(STD, dtype=torch.float64, device=x.device).view(1, 3, 1, 1)
    return (x - mean) / std


class _Net:
    """The forward with an optional calibration pass: with ``calibrate`` set, every BatchNorm's running statistics are
    set to the batch statistics of its conv output before it is applied."""

    def __init__(self, sd, calibrate=False):
        self.sd, self.calibrate = sd, calibrate

    def c(self, name, x, stride=1, padding=0):
        sd = self.sd
        y = F.conv2d(x, sd[f"{name}.conv.weight"], stride=stride, padding=padding)
        if self.calibrate:
            sd[f"{name}.bn.running_mean"] = y.mean(dim=(0, 2, 3))
            sd[f"{name}.bn.running_var"] = y.var(dim=(0, 2, 3))
        m, v = sd[f"{name}.bn.running_mean"], sd[f"{name}.bn.running_var"]
        g, b = sd[f"{name}.bn.weight"], sd[f"{name}.bn.bias"]
        y = (y - m[:, None, None]) / torch.sqrt(v + EPS)[:, None, None] * g[:, None, None] + b[:, None, None]
        return F.relu(y)

    def inception_a(self, p, x):
        b1 = self.c(f"{p}.branch1x1", x)
        b5 = self.c(f"{p}.branch5x5_2", self.c(f"{p}.branch5x5_1", x), padding=2)
        d = self.c(f"{p}.branch3x3dbl_1", x)
        d = self.c(f"{p}.branch3x3dbl_2", d, padding=1)
        d = self.c(f"{p}.branch3x3dbl_3", d, padding=1)
        bp = self.c(f"{p}.branch_pool", F.avg_pool2d(x, kernel_size=3, stride=1, padding=1))
        return torch.cat([b1, b5, d, bp], 1)

    def inception_b(self, p, x):
        b3 = self.c(f"{p}.branch3x3", x, stride=2)
        d = self.c(f"{p}.branch3x3dbl_1", x)
        d = self.c(f"{p}.branch3x3dbl_2", d, padding=1)
        d = self.c(f"{p}.branch3x3dbl_3", d, stride=2)
        return torch.cat([b3, d, F.max_pool2d(x, kernel_size=3, stride=2)], 1)

    def inception_c(self, p, x):
        b1 = self.c(f"{p}.branch1x1", x)
        b7 = self.c(f"{p}.branch7x7_1", x)
        b7 = self.c(f"{p}.branch7x7_2", b7, padding=(0, 3))
        b7 = self.c(f"{p}.branch7x7_3", b7, padding=(3, 0))
        d = self.c(f"{p}.branch7x7dbl_1", x)
        d = self.c(f"{p}.branch7x7dbl_2", d, padding=(3, 0))
        d = self.c(f"{p}.branch7x7dbl_3", d, padding=(0, 3))
        d = self.c(f"{p}.branch7x7dbl_4", d, padding=(3, 0))
        d = self.c(f"{p}.branch7x7dbl_5", d, padding=(0, 3))
        bp = self.c(f"{p}.branch_pool", F.avg_pool2d(x, kernel_size=3, stride=1, padding=1))
        return torch.cat([b1, b7, d, bp], 1)

    def inception_d(self, p, x):
        b3 = self.c(f"{p}.branch3x3_2", self.c(f"{p}.branch3x3_1", x), stride=2)
        b7 = self.c(f"{p}.branch7x7x3_1", x)
        b7 = self.c(f"{p}.branch7x7x3_2", b7, padding=(0, 3))
        b7 = self.c(f"{p}.branch7x7x3_3", b7, padding=(3, 0))
        b7 = self.c(f"{p}.branch7x7x3_4", b7, stride=2)
        return torch.cat([b3, b7, F.max_pool2d(x, kernel_size=3, stride=2)], 1)

    def inception_e(self, p, x):
        b1 = self.c(f"{p}.branch1x1", x)
        b3 = self.c(f"{p}.branch3x3_1", x)
        b3 = torch.cat([self.c(f"{p}.branch3x3_2a", b3, padding=(0, 1)), self.c(f"{p}.branch3x3_2b", b3, padding=(1, 0))], 1)
        d = self.c(f"{p}.branch3x3dbl_1", x)
        d = self.c(f"{p}.branch3x3dbl_2", d, padding=1)
        d = torch.cat([self.c(f"{p}.branch3x3dbl_3a", d, padding=(0, 1)), self.c(f"{p}.branch3x3dbl_3b", d, padding=(1, 0))], 1)
        bp = self.c(f"{p}.branch_pool", F.avg_pool2d(x, kernel_size=3, stride=1, padding=1))
        return torch.cat([b1, b3, d, bp], 1)

    def module(self, m, x):
        """Module m (include/dt_hip_inception.h numbering) on NCHW x; the last one returns [N, 2048]."""
        steps = [
            lambda x: self.c("Conv2d_1a_3x3", x, stride=2),
            lambda x: self.c("Conv2d_2a_3x3", x),
            lambda x: self.c("Conv2d_2b_3x3", x, padding=1),
            lambda x: F.max_pool2d(x, kernel_size=3, stride=2),
            lambda x: self.c("Conv2d_3b_1x1", x),
            lambda x: self.c("Conv2d_4a_3x3", x),
            lambda x: F.max_pool2d(x, kernel_size=3, stride=2),
            lambda x: self.inception_a("Mixed_5b", x),
            lambda x: self.inception_a("Mixed_5c", x),
            lambda x: self.inception_a("Mixed_5d", x),
            lambda x: self.inception_b("Mixed_6a", x),
            lambda x: self.inception_c("Mixed_6b", x),
            lambda x: self.inception_c("Mixed_6c", x),
            lambda x: self.inception_c("Mixed_6d", x),
            lambda x: self.inception_c("Mixed_6e", x),
            lambda x: self.inception_d("Mixed_7a", x),
            lambda x: self.inception_e("Mixed_7b", x),
            lambda x: self.inception_e("Mixed_7c", x),
            lambda x: F.adaptive_avg_pool2d(x, (1, 1)).flatten(1),
        ]
        return steps[m](x)


N_MODULES = 19


def run_module(sd, m, x):
    with torch.no_grad():
        return _Net(sd).module(m, x.to(torch.float64))


def features(sd, images, in_scale, in_shift):
    """[N, 2048] float64."""
    with torch.no_grad():
        net, x = _Net(sd), preprocess(images, in_scale, in_shift)
        for m in range(N_MODULES):
            x = net.module(m, x)
        return x


def random_state_dict(key_table, seed, device="cpu"):
    """float64 tensors for every key of ``key_table`` ({key: shape}): He-normal conv / fc weights, BatchNorm weight in
    [0.5, 1.5), bias in [0, 0.4) (so that about two thirds of every channel survives the ReLU), unit running stats."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, shape in key_table.items():
        if k.endswith("running_mean"):
            t = torch.zeros(shape, dtype=torch.float64)
        elif k.endswith("running_var"):
            t = torch.ones(shape, dtype=torch.float64)
        elif k.endswith("bn.weight"):
            t = 0.5 + torch.rand(shape, generator=g, dtype=torch.float64)
        elif k.endswith("bn.bias"):
            t = 0.4 * torch.rand(shape, generator=g, dtype=torch.float64)
        elif len(shape) >= 2:
            fan = 1
            for s in shape[1:]:
                fan *= s
            t = torch.randn(shape, generator=g, dtype=torch.float64) * (2.0 / fan) ** 0.5
        else:
            t = 0.01 * torch.randn(shape, generator=g, dtype=torch.float64)
        sd[k] = t.to(device)
        if k.endswith("running_var"):
            sd[k[:-len("running_var")] + "num_batches_tracked"] = torch.tensor(0, dtype=torch.long)
    return sd


def calibrate(sd, images, in_scale, in_shift):
    """Set every BatchNorm's running statistics to the batch statistics of its conv output on ``images`` (in place)."""
    with torch.no_grad():
        net, x = _Net(sd, calibrate=True), preprocess(images, in_scale, in_shift)
        for m in range(N_MODULES):
            x = net.module(m, x)
    return sd
