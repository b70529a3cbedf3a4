"""CPU reference for LCMScheduler (TEST INFRASTRUCTURE): latent-consistency sampling, epsilon prediction, no clipping or
thresholding, as diffusers 0.24 states it (diffusers itself is not a dependency here).  Written from the formulas in the form of
diffusers' `set_timesteps` / `step(model_output, timestep, sample, generator=...)`: the scheduler draws its own noise inside `step`, one
`randn` of the model output's shape per step but the last, and knows nothing of the package's coefficient or noise tables.  It has the
scheduler interface `oracle.pipeline_i2v_adapter.I2VAdapterPipeline` drives (`set_timesteps`, `timesteps`, `alphas_cumprod`,
`add_noise`, `scale_model_input`, `step` returning the latents), so `OP(unet, scheduler=ReferenceLCMScheduler(...))` is the
reference trajectory.  Noise levels and scalings in float64, the update in the latents' dtype."""
import math

import numpy as np
import torch


class ReferenceLCMScheduler:
    order = 1
    init_noise_sigma = 1.0

    def __init__(self, num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear",
                 original_inference_steps=50, timestep_scaling=10.0):
        self.T, self.original_steps, self.timestep_scaling = num_train_timesteps, original_inference_steps, timestep_scaling
        if beta_schedule == "scaled_linear":
            betas = torch.linspace(beta_start ** 0.5, beta_end ** 0.5, num_train_timesteps, dtype=torch.float32) ** 2
        else:
            betas = torch.linspace(beta_start, beta_end, num_train_timesteps, dtype=torch.float32)
        self.alphas_cumprod = torch.cumprod(1.0 - betas, dim=0)

    def set_timesteps(self, num_inference_steps, device=None):
        if num_inference_steps > self.original_steps:
            raise ValueError("more inference steps than original steps")
        k = self.T // self.original_steps
        origin = np.asarray(list(range(1, self.original_steps + 1))) * k - 1
        origin = origin[::-1].copy()
        picks = np.floor(np.linspace(0, len(origin), num=num_inference_steps, endpoint=False)).astype(np.int64)
        self.timesteps = torch.from_numpy(origin[picks].astype(np.int64))
        self.step_index = None

    def scale_model_input(self, sample, timestep=None):
        return sample

    def add_noise(self, original_samples, noise, timesteps):
        ac = self.alphas_cumprod.to(original_samples.dtype)[timesteps].flatten()
        sa, sb = ac ** 0.5, (1 - ac) ** 0.5
        while sa.dim() < original_samples.dim():
            sa, sb = sa.unsqueeze(-1), sb.unsqueeze(-1)
        return sa * original_samples + sb * noise

    @staticmethod
    def randn(shape, generator, dtype):
        """diffusers' randn_tensor on the host: one draw, or one sample per generator of a list"""
        if isinstance(generator, (list, tuple)):
            assert len(generator) == shape[0]
            return torch.cat([torch.randn((1,) + tuple(shape[1:]), generator=g, dtype=dtype) for g in generator], dim=0)
        return torch.randn(tuple(shape), generator=generator, dtype=dtype)

    def step(self, model_output, timestep, sample, eta=0.0, generator=None):
        n = len(self.timesteps)
        if self.step_index is None:              # diffusers' _init_step_index: where the (possibly truncated) loop starts
            self.step_index = int((self.timesteps == int(timestep)).nonzero()[0])
        i = self.step_index
        ac = self.alphas_cumprod.double()
        alpha_t = float(ac[int(timestep)])
        scaled = float(int(timestep)) * self.timestep_scaling                      # get_scalings_for_boundary_condition_discrete
        sigma_data = 0.5
        c_skip = sigma_data ** 2 / (scaled ** 2 + sigma_data ** 2)
        c_out = scaled / math.sqrt(scaled ** 2 + sigma_data ** 2)
        x0 = (sample - math.sqrt(1.0 - alpha_t) * model_output) / math.sqrt(alpha_t)
        denoised = c_out * x0 + c_skip * sample
        if i != n - 1:
            alpha_prev = float(ac[int(self.timesteps[i + 1])])
            noise = self.randn(model_output.shape, generator, denoised.dtype)
            prev = math.sqrt(alpha_prev) * denoised + math.sqrt(1.0 - alpha_prev) * noise
        else:
            prev = denoised
        self.step_index += 1
        return prev
