"""CPU reference for DPMSolverMultistepScheduler (TEST INFRASTRUCTURE): DPM-Solver++(2M), midpoint, epsilon prediction,
lower_order_final, as diffusers 0.24.0 states it (the version the reference's requirements pin; diffusers itself is not a
dependency here).  Written from the formulas, in the D0 / D1 form of diffusers' `multistep_dpm_solver_second_order_update`, and
independent of the package's coefficient tables.  It has the scheduler interface `oracle.pipeline_i2v_adapter.I2VAdapterPipeline`
drives (`set_timesteps`, `timesteps`, `alphas_cumprod`, `add_noise`, `scale_model_input`, `step` returning the latents), so
`OP(unet, scheduler=ReferenceDPMSolver(...))` is the reference trajectory.  Noise levels in float64, the update in the latents'
dtype."""
import math

import numpy as np
import torch


class ReferenceDPMSolver:
    order = 1
    init_noise_sigma = 1.0

    def __init__(self, num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, solver_order=2,
                 timestep_spacing="linspace", steps_offset=1, lower_order_final=True):
        self.T = num_train_timesteps
        betas = torch.linspace(beta_start ** 0.5, beta_end ** 0.5, num_train_timesteps, dtype=torch.float32) ** 2
        self.alphas_cumprod = torch.cumprod(1.0 - betas, dim=0)
        self.solver_order, self.spacing, self.steps_offset = solver_order, timestep_spacing, steps_offset
        self.lower_order_final = lower_order_final

    def set_timesteps(self, num_inference_steps, device=None):
        T, N = self.T, num_inference_steps
        if self.spacing == "linspace":
            ts = np.linspace(0, T - 1, N + 1).round()[::-1][:-1].astype(np.int64)
        elif self.spacing == "leading":
            ts = (np.arange(N + 1) * (T // (N + 1))).round()[::-1][:-1].astype(np.int64) + self.steps_offset
        else:
            ts = np.round(np.arange(T, 0, -T / N)).astype(np.int64) - 1
        self.timesteps = torch.from_numpy(ts.copy())
        ac = self.alphas_cumprod.double().numpy()
        self.sigmas = [math.sqrt((1 - ac[t]) / ac[t]) for t in ts] + [math.sqrt((1 - ac[0]) / ac[0])]
        self.step_index, self.executed, self.prev_x0 = None, 0, None

    @staticmethod
    def alpha_sigma_lambda(sigma):
        alpha = 1.0 / math.sqrt(sigma ** 2 + 1.0)
        return alpha, sigma * alpha, math.log(alpha) - math.log(sigma * alpha)

    def scale_model_input(self, sample, timestep=None):
        return sample

    def add_noise(self, original_samples, noise, timesteps):
        ac = self.alphas_cumprod.to(original_samples.dtype)[timesteps].flatten()
        sa, sb = ac ** 0.5, (1 - ac) ** 0.5
        while sa.dim() < original_samples.dim():
            sa, sb = sa.unsqueeze(-1), sb.unsqueeze(-1)
        return sa * original_samples + sb * noise

    def step(self, model_output, timestep, sample, eta=0.0, generator=None):
        n = len(self.timesteps)
        if self.step_index is None:              # diffusers' _init_step_index: where the (possibly truncated) loop starts
            self.step_index = int((self.timesteps == int(timestep)).nonzero()[0])
        i = self.step_index
        a_s0, s_s0, lam_s0 = self.alpha_sigma_lambda(self.sigmas[i])
        a_t, s_t, lam_t = self.alpha_sigma_lambda(self.sigmas[i + 1])
        x0 = (sample - s_s0 * model_output) / a_s0                       # convert_model_output (dpmsolver++, epsilon)
        h = lam_t - lam_s0
        first = (self.solver_order == 1 or self.executed < 1
                 or (self.lower_order_final and i == n - 1 and n < 15))
        if first:
            x_t = (s_t / s_s0) * sample - (a_t * (math.exp(-h) - 1.0)) * x0
        else:
            lam_s1 = self.alpha_sigma_lambda(self.sigmas[i - 1])[2]
            r0 = (lam_s0 - lam_s1) / h
            d0, d1 = x0, (1.0 / r0) * (x0 - self.prev_x0)
            x_t = (s_t / s_s0) * sample - (a_t * (math.exp(-h) - 1.0)) * d0 - 0.5 * (a_t * (math.exp(-h) - 1.0)) * d1
        self.prev_x0 = x0
        self.executed += 1
        self.step_index += 1
        return x_t
