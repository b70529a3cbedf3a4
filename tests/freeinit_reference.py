"""CPU reference for FreeInit (TEST INFRASTRUCTURE; the package never imports this): written from the formulas of diffusers 0.24
`FreeInitMixin` (`_get_free_init_freq_filter`, `_apply_freq_filter`, `_apply_free_init`), diffusers itself is not a dependency.
The filter is a triple Python loop in float64, the mix is the three-transform form with `torch.fft` in float64 on the host, and
`oracle_free_init_call` is the oracle pipeline's loop (oracle/pipeline_i2v_adapter.py) run `num_iters` times with the mix between the
rounds, drawing from the same generators in the same order as the product."""
import math

import torch

from oracle.blocks import gaussian_blur3

DIMS = (1, 3, 4)       # (frames, height, width) of the pipeline's latent layout [B, F, C, H, W]


def reference_filter(shape, method="butterworth", order=4, spatial_stop_frequency=0.25, temporal_stop_frequency=0.25):
    """float64 [F, H, W], the centred layout (index (t, h, w) multiplies frequency (t - F // 2, h - H // 2, w - W // 2))"""
    f, hh, ww = shape
    d_s, d_t = spatial_stop_frequency, temporal_stop_frequency
    mask = torch.zeros(f, hh, ww, dtype=torch.float64)
    if d_s == 0 or d_t == 0:
        return mask
    for t in range(f):
        for h in range(hh):
            for w in range(ww):
                d2 = ((d_s / d_t) * (2 * t / f - 1)) ** 2 + (2 * h / hh - 1) ** 2 + (2 * w / ww - 1) ** 2
                if method == "butterworth":
                    mask[t, h, w] = 1 / (1 + (d2 / d_s ** 2) ** order)
                elif method == "gaussian":
                    mask[t, h, w] = math.exp(-1 / (2 * d_s ** 2) * d2)
                elif method == "ideal":
                    mask[t, h, w] = 1.0 if d2 <= d_s ** 2 else 0.0
                else:
                    raise ValueError(method)
    return mask


def add_noise(latents, noise, sqrt_alpha, sqrt_one_minus_alpha):
    return sqrt_alpha * latents.double() + sqrt_one_minus_alpha * noise.double()


def reference_mix(latents, init_noise, z_rand, lpf, sqrt_alpha, sqrt_one_minus_alpha):
    """the three-transform form, float64: latents / init_noise / z_rand [B, F, C, H, W], lpf [F, H, W]"""
    z_t = add_noise(latents, init_noise, sqrt_alpha, sqrt_one_minus_alpha)
    m = lpf.double()[None, :, None]                                        # [1, F, 1, H, W]
    x_freq = torch.fft.fftshift(torch.fft.fftn(z_t, dim=DIMS), dim=DIMS)
    n_freq = torch.fft.fftshift(torch.fft.fftn(z_rand.double(), dim=DIMS), dim=DIMS)
    mixed = x_freq * m + n_freq * (1 - m)
    return torch.fft.ifftn(torch.fft.ifftshift(mixed, dim=DIMS), dim=DIMS).real


def reference_mix_one_transform(latents, init_noise, z_rand, lpf, sqrt_alpha, sqrt_one_minus_alpha, return_complex=False):
    """z_rand + Re ifftn(ifftshift(lpf) * fftn(z_t - z_rand)): the form the kernel computes"""
    z_t = add_noise(latents, init_noise, sqrt_alpha, sqrt_one_minus_alpha)
    m = torch.fft.ifftshift(lpf.double(), dim=(0, 1, 2))[None, :, None]
    back = torch.fft.ifftn(m * torch.fft.fftn(z_t - z_rand.double(), dim=DIMS), dim=DIMS)
    return back if return_complex else z_rand.double() + back.real


def randn(shape, generator, dtype=torch.float32):
    """one host draw, or one sample per generator of a list (diffusers' randn_tensor)"""
    if isinstance(generator, (list, tuple)):
        assert len(generator) == shape[0]
        return torch.cat([torch.randn((1,) + tuple(shape[1:]), generator=g, dtype=dtype) for g in generator], dim=0)
    return torch.randn(tuple(shape), generator=generator, dtype=dtype)


def round_steps(num_inference_steps, num_iters, i):
    return max(1, int(num_inference_steps / num_iters * (i + 1)))


@torch.no_grad()
def oracle_free_init_call(op, prompt_embeds, negative_prompt_embeds, condition_image_latents, *, num_iters, method="butterworth", order=4,
                          spatial_stop_frequency=0.25, temporal_stop_frequency=0.25, use_fast_sampling=False, num_frames=16,
                          num_inference_steps=50, guidance_scale=7.5, generator=None, latents=None,
                          frame_similarity_sample_ratio=1, frame_similarity_blurred_strength=0.6, prior_mask_generator=None,
                          prior_noise_generator=None, blur_sigma=None):
    """`op`: an oracle.pipeline_i2v_adapter.I2VAdapterPipeline (its unet and scheduler are used).  Round 0 is its `__call__`
    (pipe:629-700); every later round draws z_rand from `generator`, re-noises the returned clip with the prior's noise to the level of
    the round's first timestep, mixes in float64 and samples again.  Returns the last round's clip."""
    sch, cond = op.scheduler, condition_image_latents
    batch_size = prompt_embeds.shape[0]
    do_cfg = guidance_scale > 1.0
    if do_cfg:
        prompt_embeds = torch.cat([negative_prompt_embeds, prompt_embeds])
    steps_of = (lambda i: round_steps(num_inference_steps, num_iters, i)) if use_fast_sampling else (lambda i: num_inference_steps)
    sch.set_timesteps(steps_of(0))
    timesteps, _ = op.get_timesteps(steps_of(0), frame_similarity_sample_ratio)
    h_lat, w_lat = cond.shape[-2:]
    if latents is None:      # prepare_latents' draw (pipe:635-645) advances `generator`; the prior overwrites its result (pipe:656)
        randn((batch_size, num_frames, op.unet.config.in_channels, h_lat, w_lat), generator, prompt_embeds.dtype)
    if blur_sigma is None:
        blur_sigma = float(torch.empty(1).uniform_(0.1, 2.0, generator=prior_mask_generator).item())
    blurred = gaussian_blur3(cond, blur_sigma)
    exp_blur = blurred.unsqueeze(1).repeat(1, num_frames, 1, 1, 1)
    exp_cond = cond.unsqueeze(1).repeat(1, num_frames, 1, 1, 1)
    mask = (torch.rand(exp_cond.shape, generator=prior_mask_generator) < frame_similarity_blurred_strength).to(exp_cond.dtype)
    prior = mask * exp_blur + (1 - mask) * exp_cond
    init_noise = torch.randn(prior.shape, generator=prior_noise_generator, dtype=prior.dtype)
    x = sch.add_noise(prior, init_noise, timesteps[0].repeat(batch_size))
    lpf = reference_filter((num_frames, h_lat, w_lat), method, order, spatial_stop_frequency, temporal_stop_frequency)
    for rnd in range(num_iters):
        if rnd > 0:
            z_rand = randn(x.shape, generator, x.dtype)
            sch.set_timesteps(steps_of(rnd))          # (also re-arms a scheduler that counts its steps)
            timesteps, _ = op.get_timesteps(steps_of(rnd), frame_similarity_sample_ratio)
            a_t = float(sch.alphas_cumprod.double()[int(timesteps[0])])
            x = reference_mix(x, init_noise, z_rand, lpf, a_t ** 0.5, (1 - a_t) ** 0.5).to(prior.dtype)
        for t in timesteps:
            x[:, 0] = cond
            xin = torch.cat([x] * 2) if do_cfg else x
            noise_pred = op.unet(sch.scale_model_input(xin, t), t, enable_cross_frame_attn=True, encoder_hidden_states=prompt_embeds,
                                 added_cond_kwargs=None).sample
            if do_cfg:
                u, c = noise_pred.chunk(2)
                noise_pred = u + guidance_scale * (c - u)
            x = sch.step(noise_pred, t, x, eta=0.0, generator=generator)
        x[:, 0] = cond
    return x
