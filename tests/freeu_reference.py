"""FreeU reference for the tests (the oracle has no FreeU): diffusers 0.24's `fourier_filter` / `apply_freeu` restated literally with
torch.fft -- fftn, fftshift, box mask, ifftshift, ifftn(...).real -- in the dtype of the input (fp32 for the oracle's forward, fp64 for
the kernel tests), the closed four-frequency form the HIP kernel implements (include/i2v_hip.h, i2v_freeu_f16), and hooks that put
the literal form in front of the skip concatenations' consumers of an oracle UNet (the reference applies it to the two operands of
`cat([hidden, skip], 1)` of every resnet of the up blocks with resolution_idx 0 and 1, unet:453-478)."""
import math

import torch

SD15_FREEU = dict(s1=0.9, s2=0.2, b1=1.2, b2=1.4)        # the FreeU paper's SD-1.5 values


def fourier_filter(x, threshold, scale):
    """[B, C, H, W] -> the same shape and dtype: the centred (2 threshold)^2 box of the shifted spectrum times `scale`"""
    B, C, H, W = x.shape
    freq = torch.fft.fftshift(torch.fft.fftn(x, dim=(-2, -1)), dim=(-2, -1))
    mask = torch.ones((B, C, H, W), dtype=x.dtype)
    crow, ccol = H // 2, W // 2
    mask[..., crow - threshold: crow + threshold, ccol - threshold: ccol + threshold] = scale
    freq = torch.fft.ifftshift(freq * mask, dim=(-2, -1))
    return torch.fft.ifftn(freq, dim=(-2, -1)).real.to(x.dtype)


def apply_freeu(resolution_idx, hidden, skip, s1, s2, b1, b2):
    """(hidden', skip') for channel-first tensors; new tensors (the inputs are left alone)"""
    if resolution_idx in (0, 1):
        b, s = (b1, s1) if resolution_idx == 0 else (b2, s2)
        half = hidden.shape[1] // 2
        hidden = torch.cat([hidden[:, :half] * b, hidden[:, half:]], dim=1)
        skip = fourier_filter(skip, 1, s)
    return hidden, skip


def four_mode_filter(x, scale):
    """the closed form: x + (s - 1) / (H W) Re(sum over (k, l) in {0, -1}^2 of X[k, l] e^{+2 pi i (k h / H + l w / W)}), written with
    the seven real sums the kernel accumulates.  fp64."""
    x = x.double()
    H, W = x.shape[-2:]
    th = 2 * math.pi * torch.arange(H, dtype=torch.float64).view(H, 1) / H
    tw = 2 * math.pi * torch.arange(W, dtype=torch.float64).view(1, W) / W
    sm = lambda t: (x * t).sum(dim=(-2, -1), keepdim=True)
    one = torch.ones(H, W, dtype=torch.float64)
    ch, sh, cw, sw = torch.cos(th) * one, torch.sin(th) * one, torch.cos(tw) * one, torch.sin(tw) * one
    cd, sd = torch.cos(th + tw), torch.sin(th + tw)
    corr = sm(one) + sm(ch) * ch + sm(sh) * sh + sm(cw) * cw + sm(sw) * sw + sm(cd) * cd + sm(sd) * sd
    return x + (scale - 1.0) / (H * W) * corr


def tokens_reference(hidden_tok, skip_tok, b, s):
    """fp64 reference of K.freeu on token-layout tensors [N, H, W, C] (any float dtype; a pair's value is passed as fp64)"""
    hd = hidden_tok.double().permute(0, 3, 1, 2)
    sk = skip_tok.double().permute(0, 3, 1, 2)
    ho, so = apply_freeu(0, hd, sk, s1=s, s2=s, b1=b, b2=b)
    return ho.permute(0, 2, 3, 1).contiguous(), so.permute(0, 2, 3, 1).contiguous()


def hook_oracle_unet(unet, s1, s2, b1, b2):
    """forward pre-hooks on up_blocks[0 / 1].resnets[j] of an ORACLE UNet: the hook receives cat([hidden, skip], 1), splits it at
    C1 (j = 0: the previous block's output channels, else this block's), applies apply_freeu and concatenates again.  Returns the
    hook handles (`.remove()` each to switch FreeU off)."""
    handles = []
    prev_out = unet.mid_block.resnets[-1].conv2.out_channels
    for ridx, blk in enumerate(unet.up_blocks):
        out_ch = blk.resnets[-1].conv2.out_channels
        if ridx in (0, 1):
            for j, resnet in enumerate(blk.resnets):
                c1 = prev_out if j == 0 else out_ch

                def pre(_mod, args, ridx=ridx, c1=c1):
                    cat = args[0]
                    hidden, skip = apply_freeu(ridx, cat[:, :c1], cat[:, c1:], s1, s2, b1, b2)
                    return (torch.cat([hidden, skip], dim=1),) + tuple(args[1:])
                handles.append(resnet.register_forward_pre_hook(pre))
        prev_out = out_ch
    return handles
