"""FreeInit (https://arxiv.org/abs/2312.07537; diffusers 0.24 `FreeInitMixin`): host side.  The low-pass table the HIP mix reads
(`kernels.freeinit_mix`, csrc/freeinit.hip), the arguments of `I2VAdapterPipeline.enable_free_init` and the step count of a round under
`use_fast_sampling`.  The table is evaluated in float64 and rounded to fp32 once, on the host: the "ideal" filter is a `<=` on a sum of
squares, and a bin on the edge must fall where this formula puts it, not where an fp32 re-evaluation inside a kernel would."""
import torch

METHODS = ("butterworth", "gaussian", "ideal")
_tables = {}


# the largest clip `i2v_freeinit_mix` takes: frames, latent height and width (csrc/freeinit.hip FI_MAX_F / FI_MAX_HW)
MAX_FRAMES, MAX_HW = 32, 128


def free_init_filter(shape, method="butterworth", order=4, spatial_stop_frequency=0.25, temporal_stop_frequency=0.25, device=None):
    """diffusers `_get_free_init_freq_filter` for the (F, H, W) axes: fp32 [F, H, W] in the CENTRED layout (index (t, h, w) is frequency
    (t - F // 2, h - H // 2, w - W // 2), what multiplies the fftshift-ed spectrum), vectorised.  With d_s / d_t the spatial / temporal
    stop frequencies,
        d2 = ((d_s / d_t) (2 t / F - 1))^2 + (2 h / H - 1)^2 + (2 w / W - 1)^2
        butterworth 1 / (1 + (d2 / d_s^2)^order);  gaussian exp(-d2 / (2 d_s^2));  ideal 1 where d2 <= d_s^2, else 0
    and the all-zero table when either stop frequency is 0.  `device`: the table is moved there and kept per (shape, parameters, device)."""
    f, h, w = (int(v) for v in shape)
    if method not in METHODS:
        raise ValueError(f"unknown FreeInit filter {method!r}: one of {', '.join(METHODS)}")
    if min(f, h, w) < 1:
        raise ValueError(f"shape must be (F, H, W) with positive sizes, got {tuple(shape)}")
    d_s, d_t = float(spatial_stop_frequency), float(temporal_stop_frequency)
    if d_s < 0 or d_t < 0:
        raise ValueError("the stop frequencies must not be negative")
    key = (f, h, w, method, int(order), d_s, d_t, None if device is None else str(device))
    hit = _tables.get(key)
    if hit is not None:
        return hit
    if d_s == 0 or d_t == 0:
        table = torch.zeros(f, h, w, dtype=torch.float32)
    else:
        f64 = torch.float64
        t = ((d_s / d_t) * (2 * torch.arange(f, dtype=f64) / f - 1)) ** 2
        y = (2 * torch.arange(h, dtype=f64) / h - 1) ** 2
        x = (2 * torch.arange(w, dtype=f64) / w - 1) ** 2
        d2 = t[:, None, None] + y[None, :, None] + x[None, None, :]
        if method == "butterworth":
            table = 1 / (1 + (d2 / d_s ** 2) ** int(order))
        elif method == "gaussian":
            table = torch.exp(-d2 / (2 * d_s ** 2))
        else:
            table = (d2 <= d_s ** 2).to(f64)
        table = table.to(torch.float32)
    table = table.contiguous()
    if device is not None:
        table = table.to(device)
    if len(_tables) >= 16:       # a handful of shapes per process; never grows without bound
        _tables.clear()
    _tables[key] = table
    return table


def check_free_init_args(num_iters, method, order, spatial_stop_frequency, temporal_stop_frequency):
    """the argument checks of `enable_free_init`"""
    if int(num_iters) != num_iters or num_iters < 1:
        raise ValueError(f"num_iters must be an integer >= 1, got {num_iters!r}")
    if method not in METHODS:
        raise ValueError(f"unknown FreeInit filter {method!r}: one of {', '.join(METHODS)}")
    if int(order) != order or order < 1:
        raise ValueError(f"order must be an integer >= 1, got {order!r}")
    if spatial_stop_frequency < 0 or temporal_stop_frequency < 0:
        raise ValueError("the stop frequencies must not be negative")


def round_inference_steps(num_inference_steps, num_iters, i):
    """`use_fast_sampling` (diffusers `_apply_free_init`): round i of num_iters samples with this many steps, the last with all"""
    return max(1, int(num_inference_steps / num_iters * (i + 1)))
