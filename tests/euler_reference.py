"""CPU reference for EulerDiscreteScheduler and EulerAncestralDiscreteScheduler (TEST INFRASTRUCTURE): sampling in sigma space, epsilon
prediction, as diffusers 0.24 states it (diffusers itself is not a dependency here, so parity with it is unpinned: this restatement is
the specification).  Written from the formulas in the form of diffusers' `set_timesteps` / `step(model_output, timestep, sample,
generator=...)`: the ancestral scheduler draws its own noise inside `step`, one `randn` of the model output's shape per step, the last
included, and neither knows anything of the package's coefficient or noise tables.  The update keeps diffusers' written form,
derivative = (x - pred_x0) / sigma.  It has the scheduler interface `oracle.pipeline_i2v_adapter.I2VAdapterPipeline` drives
(`set_timesteps`, `timesteps`, `init_noise_sigma`, `add_noise`, `scale_model_input`, `step` returning the latents), so
`OP(unet, scheduler=ReferenceEulerScheduler(...))` is the reference trajectory.  Noise levels as fp32-rounded values used in float64,
the update in the latents' dtype."""
import numpy as np
import torch


class ReferenceEulerScheduler:
    order = 1

    def __init__(self, ancestral=False, use_karras_sigmas=False, num_train_timesteps=1000, beta_start=0.0001, beta_end=0.02,
                 beta_schedule="linear", timestep_spacing="linspace", steps_offset=0):
        assert not (ancestral and use_karras_sigmas), "diffusers 0.24's ancestral sampler has no Karras option"
        self.ancestral, self.karras = ancestral, use_karras_sigmas
        self.T, self.spacing, self.offset = num_train_timesteps, timestep_spacing, steps_offset
        if beta_schedule == "scaled_linear":
            betas = torch.linspace(beta_start ** 0.5, beta_end ** 0.5, num_train_timesteps, dtype=torch.float32) ** 2
        elif beta_schedule == "linear":
            betas = torch.linspace(beta_start, beta_end, num_train_timesteps, dtype=torch.float32)
        else:
            raise ValueError(beta_schedule)
        self.alphas_cumprod = torch.cumprod(1.0 - betas, dim=0)
        self.train_sigmas = (((1 - self.alphas_cumprod) / self.alphas_cumprod) ** 0.5).numpy().astype(np.float64)
        self.sigmas = torch.from_numpy(np.concatenate([self.train_sigmas[::-1], [0.0]]).astype(np.float32))
        self.timesteps = torch.from_numpy(np.linspace(0, self.T - 1, self.T, dtype=np.float32)[::-1].copy())
        self.step_index = None

    def sigma_to_t(self, sigma):
        """diffusers' `_sigma_to_t` for one sigma"""
        log_train = np.log(self.train_sigmas)
        log_sigma = np.log(max(sigma, 1e-10))
        dists = log_sigma - log_train[:, np.newaxis]
        low_idx = np.cumsum((dists >= 0), axis=0).argmax(axis=0).clip(max=log_train.shape[0] - 2)
        high_idx = low_idx + 1
        low, high = log_train[low_idx], log_train[high_idx]
        w = np.clip((low - log_sigma) / (low - high), 0, 1)
        return float(((1 - w) * low_idx + w * high_idx).reshape(()))

    def set_timesteps(self, num_inference_steps, device=None):
        T, n = self.T, num_inference_steps
        if self.spacing == "linspace":
            timesteps = np.linspace(0, T - 1, n, dtype=np.float32)[::-1].copy()
        elif self.spacing == "leading":
            timesteps = (np.arange(0, n) * (T // n)).round()[::-1].copy().astype(np.float32)
            timesteps += self.offset
        elif self.spacing == "trailing":
            timesteps = (np.arange(T, 0, -T / n)).round().copy().astype(np.float32)
            timesteps -= 1
        else:
            raise ValueError(self.spacing)
        sigmas = np.interp(timesteps, np.arange(0, T), self.train_sigmas)
        if self.karras:
            rho = 7.0
            lo, hi = sigmas[-1] ** (1 / rho), sigmas[0] ** (1 / rho)
            sigmas = (hi + np.linspace(0, 1, n) * (lo - hi)) ** rho
            timesteps = np.array([self.sigma_to_t(s) for s in sigmas])
        self.sigmas = torch.from_numpy(np.concatenate([sigmas, [0.0]]).astype(np.float32))
        self.timesteps = torch.from_numpy(timesteps.astype(np.float32))
        self.step_index = None

    @property
    def init_noise_sigma(self):
        top = float(self.sigmas.max())
        if self.spacing in ("linspace", "trailing"):
            return top
        return (top ** 2 + 1) ** 0.5

    def index_for(self, timestep):
        return int((self.timesteps == float(timestep)).nonzero()[0])

    def scale_model_input(self, sample, timestep):
        if self.step_index is None:              # diffusers' _init_step_index: where the (possibly truncated) loop starts
            self.step_index = self.index_for(timestep)
        sigma = float(self.sigmas[self.step_index])
        return sample / ((sigma ** 2 + 1) ** 0.5)

    def add_noise(self, original_samples, noise, timesteps):
        sigma = torch.stack([self.sigmas[self.index_for(t)] for t in timesteps.flatten()]).to(original_samples.dtype)
        while sigma.dim() < original_samples.dim():
            sigma = sigma.unsqueeze(-1)
        return original_samples + noise * sigma

    @staticmethod
    def randn(shape, generator, dtype):
        """diffusers' randn_tensor on the host: one draw, or one sample per generator of a list"""
        if isinstance(generator, (list, tuple)):
            assert len(generator) == shape[0]
            return torch.cat([torch.randn((1,) + tuple(shape[1:]), generator=g, dtype=dtype) for g in generator], dim=0)
        return torch.randn(tuple(shape), generator=generator, dtype=dtype)

    def step(self, model_output, timestep, sample, eta=0.0, generator=None):
        if self.step_index is None:
            self.step_index = self.index_for(timestep)
        sigma = float(self.sigmas[self.step_index])
        sigma_next = float(self.sigmas[self.step_index + 1])
        pred_original_sample = sample - sigma * model_output                      # epsilon prediction
        derivative = (sample - pred_original_sample) / sigma
        if not self.ancestral:
            prev = sample + derivative * (sigma_next - sigma)
        else:
            sigma_up = (sigma_next ** 2 * (sigma ** 2 - sigma_next ** 2) / sigma ** 2) ** 0.5
            sigma_down = (sigma_next ** 2 - sigma_up ** 2) ** 0.5
            prev = sample + derivative * (sigma_down - sigma)
            noise = self.randn(model_output.shape, generator, model_output.dtype)
            prev = prev + noise * sigma_up
        self.step_index += 1
        return prev
