"""A torch restatement of diffusers 0.24 `T2IAdapter(adapter_type="full_adapter")` (models/adapter.py: T2IAdapter, FullAdapter,
AdapterBlock, AdapterResnetBlock), the specification of i2v_adapter_unofficial_amd.t2i_adapter: diffusers is not installed here and
no real checkpoint has been loaded, so the module tree, the state-dict keys and the arithmetic are restated from the source.

    T2IAdapter.adapter = FullAdapter:
      unshuffle = PixelUnshuffle(8); conv_in = Conv2d(64 * in_channels, channels[0], 3, padding=1)
      body[0] = AdapterBlock(channels[0], channels[0], n, down=False); body[i] = AdapterBlock(channels[i - 1], channels[i], n, down=True)
      forward: x = conv_in(unshuffle(x)); for b in body: x = b(x); features.append(x)
    AdapterBlock: downsample = AvgPool2d(2, stride=2, ceil_mode=True) if down; in_conv = Conv2d(cin, cout, 1) if cin != cout;
      resnets = Sequential(n x AdapterResnetBlock(cout));   forward: downsample -> in_conv -> resnets
    AdapterResnetBlock: block1 = Conv2d(c, c, 3, padding=1); act = ReLU; block2 = Conv2d(c, c, 1);   forward: block2(act(block1(x))) + x

It runs on the CPU in fp32 (or any dtype).  `small_*` are the shapes and weights the tests share.
"""
import torch
from torch import nn

SMALL_CHANNELS = (32, 64, 128, 128)      # the small UNet's block_out_channels (tests/parity.SMALL_UNET)


class AdapterResnetBlock(nn.Module):
    def __init__(self, channels):
        super().__init__()
        self.block1 = nn.Conv2d(channels, channels, kernel_size=3, padding=1)
        self.act = nn.ReLU()
        self.block2 = nn.Conv2d(channels, channels, kernel_size=1)

    def forward(self, x):
        return self.block2(self.act(self.block1(x))) + x


class AdapterBlock(nn.Module):
    def __init__(self, in_channels, out_channels, num_res_blocks, down=False):
        super().__init__()
        self.downsample = nn.AvgPool2d(kernel_size=2, stride=2, ceil_mode=True) if down else None
        self.in_conv = nn.Conv2d(in_channels, out_channels, kernel_size=1) if in_channels != out_channels else None
        self.resnets = nn.Sequential(*[AdapterResnetBlock(out_channels) for _ in range(num_res_blocks)])

    def forward(self, x):
        if self.downsample is not None:
            x = self.downsample(x)
        if self.in_conv is not None:
            x = self.in_conv(x)
        return self.resnets(x)


class FullAdapter(nn.Module):
    def __init__(self, in_channels=3, channels=(320, 640, 1280, 1280), num_res_blocks=2, downscale_factor=8):
        super().__init__()
        self.unshuffle = nn.PixelUnshuffle(downscale_factor)
        self.conv_in = nn.Conv2d(in_channels * downscale_factor ** 2, channels[0], kernel_size=3, padding=1)
        self.body = nn.ModuleList([AdapterBlock(channels[0], channels[0], num_res_blocks)] +
                                  [AdapterBlock(channels[i - 1], channels[i], num_res_blocks, down=True) for i in range(1, len(channels))])
        self.total_downscale_factor = downscale_factor * 2 ** (len(channels) - 1)

    def forward(self, x):
        x = self.conv_in(self.unshuffle(x))
        features = []
        for block in self.body:
            x = block(x)
            features.append(x)
        return features


class T2IAdapter(nn.Module):
    def __init__(self, in_channels=3, channels=(320, 640, 1280, 1280), num_res_blocks=2, downscale_factor=8, adapter_type="full_adapter"):
        super().__init__()
        if adapter_type != "full_adapter":
            raise ValueError(f"only full_adapter is restated, got {adapter_type}")
        self.adapter = FullAdapter(in_channels, channels, num_res_blocks, downscale_factor)

    def forward(self, x):
        return self.adapter(x)


def small_config(in_channels=3):
    return dict(in_channels=in_channels, channels=SMALL_CHANNELS, num_res_blocks=2, downscale_factor=8, adapter_type="full_adapter")


def small_reference(in_channels=3, seed=11):
    """the small adapter with torch's default initialisation under a fixed seed, its weights rounded to fp16 (so that the HIP model,
    which stores fp16, holds the same numbers)"""
    torch.manual_seed(seed)
    m = T2IAdapter(**small_config(in_channels)).eval()
    with torch.no_grad():
        for p in m.parameters():
            p.copy_(p.half().float())
    return m


def small_frames(in_channels, height, width, batch=2, seed=3):
    """control frames in [0, 1], representable in fp16"""
    g = torch.Generator().manual_seed(seed)
    return torch.rand(batch, in_channels, height, width, generator=g).half().float()


def feature_sizes(height, width):
    """(h, w) of the four feature maps for an image of height x width pixels: H / 8, then the ceil halves"""
    h, w = height // 8, width // 8
    out = []
    for _ in range(4):
        out.append((h, w))
        h, w = (h + 1) // 2, (w + 1) // 2
    return out
