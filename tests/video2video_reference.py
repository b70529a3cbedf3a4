"""Video-to-video and masked editing, restated in fp32 on the CPU (TEST INFRASTRUCTURE): the specification the pipeline's `video=` /
`strength=` / `mask_image=` and the kernel i2v_masked_renoise_f32 are held to.

diffusers is not installed here, so the two diffusers behaviours are restated from their definition:
  * AnimateDiffVideoToVideoPipeline: `get_timesteps(num_inference_steps, strength)` keeps the last
    min(int(num_inference_steps * strength), num_inference_steps) timesteps of the schedule, and the initial latents are
    scheduler.add_noise(video_latents, noise, timesteps[0]) = sqrt(abar) * video_latents + sqrt(1 - abar) * noise;
  * the inpainting pipelines' update for a 4-channel UNet (StableDiffusionInpaintPipeline, `num_channels_unet == 4`): after every
    scheduler step,  latents = (1 - m) * add_noise(source, noise, t_{i+1}) + m * latents,  after the last step
    (1 - m) * source + m * latents, with the SAME initial noise; m = 1 regenerates, m = 0 keeps the source.  The mask is converted to
    grey, resized, binarised at 0.5 and taken to the latent resolution by torch.nn.functional.interpolate (nearest).

The coefficient table's convention (include/i2v_hip.h): the scheduler-step kernels advance the device step counter before the blend
reads it and wrap it to 0 after the last step, so row 0 is (1, 0) -- the clean source -- and row r >= 1 is the noise level of
timesteps[r].

Every function computes in the dtype of its inputs: the tests call `blend` in float64 on the kernel's fp32 operands to get a reference
whose own rounding does not count against the kernel.
"""
import numpy as np
import torch
import torch.nn.functional as F

EPS32 = 2.0 ** -24          # the relative error of one fp32 rounding


# ---------------------------------------------------------------------------------------------------------- schedule
def alphas_cumprod(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012):
    """the SD-1.5 schedule ("scaled_linear") every scheduler of the project defaults to, fp32"""
    betas = torch.linspace(beta_start ** 0.5, beta_end ** 0.5, num_train_timesteps, dtype=torch.float32) ** 2
    return torch.cumprod(1.0 - betas, dim=0)


def get_timesteps(timesteps, num_inference_steps, strength):
    """the tail of the schedule that runs: (timesteps[t_start:], number of steps)"""
    init_timestep = min(int(num_inference_steps * strength), num_inference_steps)
    t_start = max(num_inference_steps - init_timestep, 0)
    return timesteps[t_start:], num_inference_steps - t_start


def noise_level(ac, t):
    """(sqrt(abar_t), sqrt(1 - abar_t)) as `add_noise` computes them, in fp32"""
    a = ac[int(t)].to(torch.float32)
    return float(a ** 0.5), float((1 - a) ** 0.5)


def add_noise(source, noise, ac, t):
    sa, sb = noise_level(ac, t)
    return sa * source + sb * noise


def initial_latents(source, noise, ac, t0):
    """video-to-video starts from the source at the first executed timestep's noise level"""
    return add_noise(source, noise, ac, t0)


def renoise_table(ac, timesteps):
    """fp32 [len(timesteps), 2]: row 0 = (1, 0); row r >= 1 = noise_level(timesteps[r])"""
    rows = [(1.0, 0.0)] + [noise_level(ac, t) for t in list(timesteps)[1:]]
    return torch.tensor(rows, dtype=torch.float32)


# ---------------------------------------------------------------------------------------------------------- mask
def prepare_mask(mask, batch_size, num_frames, height, width, scale=8):
    """-> fp32 [B, F, 1, height / 8, width / 8].  mask: a PIL image or [H, W] tensor (all frames), a list of PIL images, [F, 1, H, W] or
    [B, F, 1, H, W]; values in [0, 1].  grey -> height x width (PIL: Lanczos, tensors: nearest) -> (>= 0.5) -> nearest to the latent
    size.  A tensor already at the latent size is taken as it is."""
    import PIL.Image
    h, w = height // scale, width // scale
    if isinstance(mask, PIL.Image.Image):
        mask = [mask]
    if isinstance(mask, (list, tuple)):
        planes = []
        for im in mask:
            im = im.convert("L")
            if im.size != (width, height):
                im = im.resize((width, height), resample=PIL.Image.LANCZOS)
            planes.append(torch.from_numpy(np.asarray(im, dtype=np.float32) / 255.0))
        t = torch.stack(planes)[None, :, None]
    else:
        t = mask.detach().float()
        t = t[None, None, None] if t.dim() == 2 else (t[None] if t.dim() == 4 else t)
    out = torch.empty(batch_size, num_frames, 1, h, w)
    for b in range(batch_size):
        for f in range(num_frames):
            plane = t[b if t.shape[0] > 1 else 0, f if t.shape[1] > 1 else 0][None]          # [1, 1, H, W]
            if tuple(plane.shape[-2:]) != (h, w):
                if tuple(plane.shape[-2:]) != (height, width):
                    plane = F.interpolate(plane, size=(height, width), mode="nearest")
                plane = F.interpolate((plane >= 0.5).float(), size=(h, w), mode="nearest")
            out[b, f] = plane[0]
    return out


# ---------------------------------------------------------------------------------------------------------- the blend
def blend(latents, source, noise, mask, a, b):
    """m * latents + (1 - m) * (a * source + b * noise); latents / source / noise [..., C, H, W], mask [..., 1, H, W] (broadcast over
    the channels).  In the inputs' dtype."""
    return mask * latents + (1 - mask) * (a * source + b * noise)


def blend_bound(latents, source, noise, mask, a, b):
    """the kernel's per-element error bound: 4 * 2^-24 * (|m l| + |1 - m| (|a s| + |b n|)) -- a handful of fp32 roundings of those
    terms, whatever the contraction.  float64."""
    l, s, n, m = (t.double() for t in (latents, source, noise, mask))
    return 4 * EPS32 * ((m * l).abs() + (1 - m).abs() * ((a * s).abs() + (b * n).abs()))


def check_blend(got, latents, source, noise, mask, a, b):
    """(worst |got - ref| / bound over the elements with a positive bound, everything inside the bound) against the float64 blend of
    the fp32 operands; where the bound is 0 the result must be exactly the reference"""
    l, s, n, m = (t.double() for t in (latents, source, noise, mask))
    ref = blend(l, s, n, m, float(a), float(b))
    bound = blend_bound(latents, source, noise, mask, float(a), float(b))
    err = (got.double() - ref).abs()
    ok = bool((err <= bound).all()) and bool(torch.isfinite(got).all())
    pos = bound > 0
    worst = float((err[pos] / bound[pos]).max()) if pos.any() else 0.0
    if not bool((err[~pos] == 0).all()):
        worst = float("inf")
    return worst, ok


# ---------------------------------------------------------------------------------------------------------- the sampling loop
@torch.no_grad()
def sample(unet, prompt_embeds, negative_prompt_embeds, cond, source, noise, num_inference_steps, strength, guidance_scale=7.5, mask=None,
           callback=None):
    """DDIM video-to-video on the oracle's UNet: add_noise to the first executed timestep, then per step the frame-0 overwrite, the CFG
    UNet call, the scheduler step and -- with a mask [B, F, 1, h, w] -- the blend; the frame-0 overwrite once more at the end.
    callback(i, t, latents) sees the latents after step i's blend."""
    from oracle.blocks import DDIMScheduler
    sched = DDIMScheduler()
    sched.set_timesteps(num_inference_steps)
    timesteps, _ = get_timesteps(sched.timesteps, num_inference_steps, strength)
    ac = sched.alphas_cumprod
    latents = initial_latents(source, noise, ac, timesteps[0])
    table = renoise_table(ac, timesteps)
    ctx = torch.cat([negative_prompt_embeds, prompt_embeds])
    for i, t in enumerate(timesteps):
        latents[:, 0] = cond
        pred = unet(torch.cat([latents] * 2), t, enable_cross_frame_attn=True, encoder_hidden_states=ctx).sample
        u, c = pred.chunk(2)
        latents = sched.step(u + guidance_scale * (c - u), t, latents, eta=0.0)
        if mask is not None:
            a, b = table[(i + 1) % len(timesteps)]
            latents = blend(latents, source, noise, mask, float(a), float(b))
        if callback is not None:
            callback(i, t, latents.clone())
    latents[:, 0] = cond
    return latents
