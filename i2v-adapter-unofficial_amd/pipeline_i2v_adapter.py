"""I2VAdapterPipeline denoising loop on the HIP kernels: drop-in for the hot part of
/root/reference/src/pipelines/pipeline_i2v_adapter.py (`__init__` pipe:75-112, `prepare_latents` :265-297,
`get_timesteps` :529-536, `__call__` :538-719, loop :663-700).

One DDIM step = frame-0 overwrite + CFG duplicate + layout edge (i2v_ddim_prep), timestep embedding, the UNet,
CFG combine + DDIM update (i2v_ddim_cfg_step; with a DPMSolverMultistepScheduler the DPM-Solver++(2M) update,
i2v_dpm_cfg_step, which also keeps the previous data prediction on the device; with an LCMScheduler the latent-consistency update,
i2v_lcm_cfg_step, which re-noises with this step's row of a noise table drawn once per sample; with this package's EulerDiscreteScheduler /
EulerAncestralDiscreteScheduler the prep scales the model input, i2v_sigma_prep, and the update is i2v_euler_cfg_step, the ancestral
sampler's noise from such a table too).  The whole step is captured ONCE as a hipGraph (through
torch.cuda.CUDAGraph on the stream the ctypes launches go to) and replayed for every timestep: the step's
scalars (t, sqrt(a_t), ...) are read on the device from small tables indexed by a device-side step counter, so
there is no per-step host<->device traffic and no per-step sync (the reference syncs once per step on
`alphas_cumprod[t]`).

Either side of the loop: the condition image is encoded and the final latents are decoded by the HIP
AutoencoderKL (vae.py: pipe:300-320, 626-627) when a `vae` is given; pre / post-processing, `tensor2vid` and GIF
export are host-side plumbing (image_processor.py).  A `prompt` is encoded by the HIP CLIP text encoder (clip_text.py, `encode_prompt`
pipe:348-527) when the pipeline holds a `text_encoder` and a `tokenizer`; `prompt_embeds` / `negative_prompt_embeds` are taken as given.
`ip_adapter_image` is encoded by `encode_image` (same as pipe:323-345) when the pipeline holds an `image_encoder`
(clip_vision.CLIPVisionModelWithProjection; `load_ip_adapter` loads it from `<path>/<subfolder>/image_encoder`) and the UNet an
IP-Adapter; `image_embeds` / `negative_image_embeds` are taken as given.
"""
import contextlib
import logging
import os
from typing import Optional

import torch

from . import blocks
from . import kernels as K
from ._lib import HipLibraryError
from .blocks import (DDIMScheduler, DPMSolverMultistepScheduler, EulerAncestralDiscreteScheduler, EulerDiscreteScheduler, ImageProjection,
                     LCMScheduler, Resampler)
from .image_processor import VaeImageProcessor, tensor2vid
from .unet_motion_cross_frame_attn import UNetMotionCrossFrameAttnModel

# The two classifier-free-guidance halves of a step's batch are the same latents at the same timestep until the first text
# cross-attention: that prefix of the UNet is computed once (same numbers bit for bit; I2V_CFG_SHARED=0 computes it twice,
# as the reference does).
CFG_SHARED = os.environ.get("I2V_CFG_SHARED", "1") != "0"

f16 = torch.float16
logger = logging.getLogger(__name__)

# diffusers schedulers the reference's pipeline accepts (pipe:25-32, 83-90) that this build refuses by class name.  Only LMS and PNDM are
# unsupported in principle (each needs 3-4 history tensors the captured step has no room for); the two Euler names are refused for a
# FOREIGN object of that name (diffusers' own class: its tables are not this build's) -- this package's EulerDiscreteScheduler and
# EulerAncestralDiscreteScheduler (blocks.py) run, recognised by isinstance before the name check
UNSUPPORTED_SCHEDULERS = ("EulerDiscreteScheduler", "EulerAncestralDiscreteScheduler", "LMSDiscreteScheduler", "PNDMScheduler")


class I2VAdapterPipelineOutput:
    def __init__(self, frames):
        self.frames = frames


def draw_blur_sigma(generator=None, sigma_min: float = 0.1, sigma_max: float = 2.0) -> float:
    """torchvision GaussianBlur(kernel_size=3) (pipe:112) draws sigma ~ U(0.1, 2.0) once per call
    (`GaussianBlur.get_params`); the reference uses the unseeded global RNG, here the draw takes a generator."""
    gdev = generator.device if generator is not None else torch.device("cpu")
    return float(torch.empty(1, device=gdev).uniform_(sigma_min, sigma_max, generator=generator).item())


def _draw(fn, shape, generator, device):
    """one seeded draw on the generator's own device (host generators reproduce the CPU oracle's numbers bit for bit;
    a torch.Generator(device="cuda") keeps the whole prior on the GPU), moved to `device`.  A list of generators draws
    one sample (leading index) per generator, as `prepare_latents` does (pipe:287-290): a sample's noise then does not
    depend on which other samples share its call."""
    if isinstance(generator, (list, tuple)):
        if len(generator) != shape[0]:
            raise ValueError(f"{len(generator)} generators for a batch of {shape[0]}")
        return torch.cat([_draw(fn, (1,) + tuple(shape[1:]), g, device) for g in generator], dim=0)
    gdev = generator.device if generator is not None else torch.device("cpu")
    return fn(shape, generator=generator, dtype=torch.float32, device=gdev).to(device)


# The per-sample device buffers a captured step reads, by their key in the state dict `st`: each a tensor, a tuple of tensors
# (t2i_feats; cn_cond with a MultiControlNetModel, one per net) or absent / None.  The ONE list of them: a graph-cache hit copies exactly these into the graph's static buffers
# (`_copy_sample_inputs`, in this order) and `_graph_key` holds the shape and dtype of exactly these, so what is copied in always
# fits.  Not listed: `x0_prev` (DPM-Solver++) is the step's own history, not a sample input -- the first step of a sample does not
# read it; `ctx_proj`, `temb_table` and the ControlNet's pair are projected from these into the static buffers (`_project_once`).
SAMPLE_INPUTS = ("latents", "cond", "t_table", "coef", "ctx_text", "ctx_ip", "noise",      # (noise: this sample's LCM / Euler-a draws)
                 "cn_cond", "cn_scale", "t2i_scale",                                       # (this sample's control frames)
                 "v2v_source", "v2v_noise", "v2v_mask", "v2v_coef",                        # (this sample's clip and mask)
                 "t2i_feats")                                                              # (this sample's adapter features)


def _copy_sample_inputs(gst, st):
    """a graph-cache hit: this sample's inputs `st` into the static buffers `gst` of the captured step, in place (the graph keeps
    reading the same memory), and the step counter back to 0.  Entries `st` does not hold are left as they are."""
    for name in SAMPLE_INPUTS:
        src = st.get(name)
        if src is None:
            continue
        for dst, t in zip(gst[name], src) if isinstance(src, (tuple, list)) else ((gst[name], src),):
            dst.copy_(t)
    gst["step_idx"].zero_()


def _sample_input_shapes(st):
    """the shape and dtype of every entry of SAMPLE_INPUTS (None where `st` holds none): their part of the graph key"""
    one = lambda t: (tuple(t.shape), t.dtype)
    shp = lambda v: None if v is None else tuple(one(t) for t in v) if isinstance(v, (tuple, list)) else one(v)
    return tuple(shp(st.get(name)) for name in SAMPLE_INPUTS)


_UNSET = object()      # an argument that was not passed, where None is a value of its own (`enable_hires_fix(scale=...)`)


@contextlib.contextmanager
def _set_for_call(setter, value):
    """`setter(value)` now and `setter(previous)` on the way out, exceptions included; `setter` returns the value it replaces"""
    prev = setter(value)
    try:
        yield
    finally:
        setter(prev)


def _frame_count(frames, name, channels, channel_owner=None):
    """the number of frames of a per-frame image input: a list of PIL images, [F, C, H, W] shared by the batch or [B, F, C, H, W].
    ValueError for anything else and for a tensor whose channel count is not `channels` -- worded "`name` has n channels, {channel_owner}
    is C" where a model decides C (the adapter's `in_channels`), else by the accepted layouts."""
    if isinstance(frames, torch.Tensor):
        if frames.dim() not in (4, 5) or (channel_owner is None and frames.shape[-3] != channels):
            raise ValueError(f"`{name}` must be [F, {channels}, H, W] or [B, F, {channels}, H, W], got {tuple(frames.shape)}")
        if frames.shape[-3] != channels:
            raise ValueError(f"`{name}` has {frames.shape[-3]} channels, {channel_owner} is {channels}")
        return frames.shape[-4]
    if isinstance(frames, (list, tuple)):
        return len(frames)
    raise ValueError(f"`{name}` must be a list of `num_frames` images or a tensor, got {type(frames)}")


def _frame_tensor(frames, name, height, width, batch_size=None, num_frames=None, channels=None, channel_owner=None):
    """a per-frame image input given as a tensor -> fp32 [B, F, C, height, width] on the host, values untouched.  With `batch_size`,
    [F, C, H, W] is expanded over the batch and the batch and frame counts are checked (without: [1, F, C, H, W], the caller
    expands); `channel_owner` as in `_frame_count`; the frames must already have the size."""
    t = frames.detach().float().cpu()
    if t.dim() == 4:
        t = t[None] if batch_size is None else t[None].expand(batch_size, -1, -1, -1, -1)
    if batch_size is not None and (t.shape[0] != batch_size or t.shape[1] != num_frames):
        raise ValueError(f"`{name}` {tuple(frames.shape)} does not match batch {batch_size} x {num_frames} frames")
    if channel_owner is not None and t.shape[2] != channels:
        raise ValueError(f"`{name}` has {t.shape[2]} channels, {channel_owner} is {channels}")
    if tuple(t.shape[-2:]) != (height, width):
        raise ValueError(f"`{name}` tensors must already be {height} x {width}, got {tuple(t.shape[-2:])}")
    return t


def _pil_plane(im, name, mode, height, width):
    """one PIL image of the list `name` -> fp32 [height, width] ("L") or [height, width, 3] ("RGB") in [0, 1], Lanczos-resized"""
    import numpy as np
    import PIL.Image
    if not isinstance(im, PIL.Image.Image):
        raise ValueError(f"`{name}` as a list holds PIL images, got {type(im)}")
    im = im.convert(mode)
    if im.size != (width, height):
        im = im.resize((width, height), resample=PIL.Image.LANCZOS)
    return torch.from_numpy(np.asarray(im, dtype=np.float32) / 255.0)


class I2VAdapterPipeline:
    """Reference constructor order (pipe:75-93): (vae, text_encoder, tokenizer, unet, motion_adapter, i2v_adapter,
    scheduler, feature_extractor, image_encoder).  `unet` may be an SD-1.5-layout `UNet2DConditionModel` container
    (then the motion UNet is assembled with `from_unet2d`, pipe:96) or an already built
    `UNetMotionCrossFrameAttnModel`."""

    vae_scale_factor = 8
    model_cpu_offload_seq = "text_encoder->image_encoder->unet->vae"

    def __init__(self, vae=None, text_encoder=None, tokenizer=None, unet=None, motion_adapter=None,
                 i2v_adapter=None, scheduler=None, feature_extractor=None,
                 image_encoder=None, controlnet=None, t2i_adapter=None):
        if unet is None:
            raise ValueError("`unet` is required")
        if isinstance(controlnet, (list, tuple)):
            raise NotImplementedError("a list of ControlNets is not taken as it is: wrap it, `MultiControlNetModel([a, b])`")
        self.controlnet = controlnet
        if isinstance(t2i_adapter, (list, tuple)):
            raise NotImplementedError("a list of T2I-Adapters (diffusers' MultiAdapter) is not implemented: pass one T2IAdapter")
        self.t2i_adapter = t2i_adapter
        if not isinstance(unet, UNetMotionCrossFrameAttnModel):
            unet = UNetMotionCrossFrameAttnModel.from_unet2d(unet, motion_adapter, i2v_adapter)     # pipe:96
        self.unet = unet
        self.vae, self.text_encoder, self.tokenizer = vae, text_encoder, tokenizer
        self.motion_adapter, self.i2v_adapter = motion_adapter, i2v_adapter
        self.scheduler = scheduler if scheduler is not None else DDIMScheduler()
        self._scheduler_kind()
        self.feature_extractor, self.image_encoder = feature_extractor, image_encoder
        if vae is not None:                                                                  # pipe:110-111
            self.vae_scale_factor = 2 ** (len(vae.config["block_out_channels"]) - 1)
        self.image_processor = VaeImageProcessor(vae_scale_factor=self.vae_scale_factor)
        # control images stay in [0, 1] (diffusers' control_image_processor: do_normalize=False)
        self.control_image_processor = VaeImageProcessor(vae_scale_factor=self.vae_scale_factor, do_normalize=False)
        self._vae_slicing = False
        self._graph = None
        self._graph_cache = {}
        self._free_init = None
        self._hires_fix = None
        self._upscaler = None
        self._prompt_weighting = None
        self._textual_inversions = []

    # ------------------------------------------------------------------------------------------ textual inversion
    def load_textual_inversion(self, pretrained_model_name_or_path_or_dict, token=None, weight_name=None, subfolder=None):
        """diffusers' `TextualInversionLoaderMixin.load_textual_inversion` (textual_inversion.py): a file (`.safetensors`,
        or `.bin` / `.pt` through `torch.load(..., weights_only=True)`), a directory plus `weight_name`, a state dict, or a list of
        these with a list of `token`.  Formats: {token: tensor [D] or [n, D]} with one key (diffusers) and {"string_to_param": {"*":
        tensor [n, D]}, "name": str} (A1111); `token` overrides the file's.  n vectors add the tokens tok, tok_1, ... tok_{n-1} to the
        tokenizer and n rows to the text encoder's token table (`CLIPTextModel.resize_token_embeddings`).  ValueError, with nothing
        modified: an embedding whose width is not the text encoder's hidden size, a token (or one of its multi-vector names) the
        tokenizer already has, a pipeline without text encoder or tokenizer, several keys without `token`."""
        from . import textual_inversion as TI
        TI.load(self, pretrained_model_name_or_path_or_dict, token=token, weight_name=weight_name, subfolder=subfolder)

    def unload_textual_inversion(self, tokens=None):
        """diffusers' `unload_textual_inversion`: all loaded inversions, or those whose token is in `tokens`.  With all of them gone the
        token table and `config.vocab_size` are the original ones, bit for bit.  A tokenizer with `remove_tokens(list)` gives the ids
        back (inversions that stay are re-added at compact ids); transformers' CLIPTokenizer cannot remove a token, so there the ids
        stay RESERVED in the tokenizer -- an unloaded token's text still tokenises to its ids, which are past the table, and encoding
        it raises -- and the table keeps its rows up to the last id still loaded."""
        from . import textual_inversion as TI
        TI.unload(self, tokens)

    def maybe_convert_prompt(self, prompt, tokenizer):
        """diffusers' `maybe_convert_prompt` (pipe:409, 491): every multi-vector token the tokenizer finds in the prompt (a str or a
        list of str) is written out as `tok tok_1 ... tok_{n-1}`.  The prompt itself, unchanged, when nothing is loaded."""
        from . import textual_inversion as TI
        return TI.convert_prompt(self, prompt, tokenizer)

    # ------------------------------------------------------------------------------------------ weighted and long prompts
    def enable_prompt_weighting(self, max_embeddings_multiples: int = 3, restore_mean: bool = True):
        """Weighted and long prompts (prompt_weighting.py): while enabled, `__call__` and `encode_prompt_travel` encode
        through `encode_weighted_prompt` -- `(text)` x 1.1, `[text]` / 1.1, `(text:1.5)`, nested and escaped as in the SD-1.5 front
        ends -- and a prompt may fill up to `max_embeddings_multiples` chunks of `model_max_length - 2` tokens (3: 225 tokens, a
        context of 231 rows).  restore_mean: every prompt is rescaled to the mean it had before the weights.  A context longer than
        `model_max_length` leaves the fused text cross-attention for `i2v_attention_f16` (README: the measured price).  The longest
        context that path takes is `prompt_weighting.max_context_tokens()` -- 419 302 tokens at SD-1.5's 1280-wide K, from
        i2v_attention_f16's 32-bit addressing of one K slice -- and a setting that can exceed it raises ValueError."""
        from . import prompt_weighting as PW
        PW.check_settings(max_embeddings_multiples, restore_mean)
        if self.tokenizer is not None:
            self._check_context_length(max_embeddings_multiples * self.tokenizer.model_max_length)
        self._prompt_weighting = dict(max_embeddings_multiples=max_embeddings_multiples, restore_mean=restore_mean)

    def disable_prompt_weighting(self):
        self._prompt_weighting = None

    @property
    def prompt_weighting_enabled(self):
        return self._prompt_weighting is not None

    def _check_context_length(self, tokens):
        from .prompt_weighting import max_context_tokens
        cfg = getattr(self.unet, "config", None)
        widest = max(getattr(cfg, "block_out_channels", None) or (1280,))
        limit = max_context_tokens(widest)
        if tokens > limit:
            raise ValueError(f"a text context of {tokens} tokens exceeds the {limit} that the cross-attention takes (i2v_attention_f16 "
                             f"addresses one K slice of {widest}-wide rows with 32 bits): lower `max_embeddings_multiples`")

    def _require_text_encoder(self):
        """the two refusals of everything that encodes text here: no text encoder or tokenizer, a text encoder that wants padding masks"""
        if self.text_encoder is None or self.tokenizer is None:
            raise ValueError("encoding a `prompt` needs both a `text_encoder` and a `tokenizer`: build the pipeline with them, or pass "
                             "`prompt_embeds` (and `negative_prompt_embeds`)")
        if getattr(self.text_encoder.config, "use_attention_mask", None):
            raise NotImplementedError("text_encoder.config.use_attention_mask: padding attention masks are not implemented")

    def _embed_ids(self, ids, clip_skip=None):
        """the text encoder's embeddings [N, L, D] of token ids [N, L]: its last hidden state, or with `clip_skip` the hidden state
        `clip_skip` layers earlier, `hidden_states[-(clip_skip + 1)]`, through the final LayerNorm -- which the last hidden state has
        been through as well (pipe:445-453)"""
        if clip_skip is None:
            return self.text_encoder(ids, attention_mask=None)[0]
        hidden = self.text_encoder(ids, attention_mask=None, output_hidden_states=True)[-1][-(clip_skip + 1)]
        return self.text_encoder.text_model.final_layer_norm(hidden)

    def _encode_weighted_texts(self, groups, clip_skip=None):
        """[sum(len(g)), n * M, D]: the weighted embeddings of lists of prompts, every list through the text encoder in one call of
        [len(g) * n, M] ids (chunks in prompt-major order); n, the chunk count, is the largest any text of ANY list needs.  One
        `K.weight_embeds` launch, in place, for all of them, and one read of the ratios."""
        from . import prompt_weighting as PW
        self._require_text_encoder()
        cfg = self._prompt_weighting or dict(max_embeddings_multiples=3, restore_mean=True)
        tok, m = self.tokenizer, self.tokenizer.model_max_length
        bos, eos, pad = PW.special_ids(tok)
        flat = [t for g in groups for t in g]
        if not flat or not all(isinstance(t, str) for t in flat):
            raise ValueError("a weighted prompt is a str (or a list of str)")
        pairs = [PW.truncate(tok, *PW.token_weights(tok, self.maybe_convert_prompt(t, tok)), m, cfg["max_embeddings_multiples"])
                 for t in flat]
        n = max(PW.chunks_needed(len(ids), m) for ids, _ in pairs)
        self._check_context_length(n * m)
        rows = [PW.chunk(ids, w, m, bos, eos, pad, n) for ids, w in pairs]
        embeds, first = [], 0
        for g in groups:
            ids = torch.tensor([r for id_rows, _ in rows[first: first + len(g)] for r in id_rows], dtype=torch.int64)
            first += len(g)
            e = self._embed_ids(ids, clip_skip)
            embeds.append(e.reshape(len(g), n * m, e.shape[-1]))
        src = (embeds[0] if len(embeds) == 1 else torch.cat(embeds)).contiguous()
        if src.dtype != f16:
            raise HipLibraryError(f"prompt weighting scales fp16 embeddings (i2v_weight_embeds_f16), the text encoder gives {src.dtype}")
        weights = torch.tensor([[x for r in w_rows for x in r] for _, w_rows in rows], dtype=torch.float32).to(src.device)
        out, ratio = K.weight_embeds(src, weights, restore_mean=cfg["restore_mean"], out=src)
        bad = (~torch.isfinite(ratio.cpu())).nonzero()
        if bad.numel():
            i = int(bad[0])
            raise ValueError(f"prompt weighting: the weights of prompt {i} ({flat[i]!r}) cancel the mean of its embedding (the ratio "
                             "unweighted mean / weighted mean is not finite): change the weights, or "
                             "enable_prompt_weighting(restore_mean=False)")
        return out

    def encode_weighted_prompt(self, prompt, device, num_videos_per_prompt, do_classifier_free_guidance, negative_prompt=None,
                               clip_skip=None):
        """`encode_prompt` for weighted and long prompts: (prompt_embeds, negative_prompt_embeds), each [B * num_videos_per_prompt,
        n * M, D] with M the tokenizer's `model_max_length` and n the chunk count of the longest text of the call, the negative
        prompts included (None without classifier-free guidance).  Textual-inversion conversion first, then
        `prompt_weighting.parse_prompt_attention`, every segment tokenised on its own, chunks of [bos] + M - 2 ids + [eos] + [pad]...,
        ids beyond `max_embeddings_multiples` chunks dropped with a warning.  The prompts' chunks go through the text encoder in one
        call and the negative prompts' in another -- the calls `encode_prompt` makes, so an unweighted prompt of at most M - 2 tokens
        gives `encode_prompt`'s embeddings bit for bit (the library's GEMM routes depend on the row count) -- and ONE
        `i2v_weight_embeds_f16` launch weighs all of them.  `clip_skip` as in `encode_prompt`.  ValueError: weights that cancel a
        prompt's mean under `restore_mean`.  Works whether or not weighting is enabled (`enable_prompt_weighting` holds the settings;
        the defaults otherwise)."""
        if isinstance(prompt, str):
            prompts = [prompt]
        elif isinstance(prompt, (list, tuple)) and prompt:
            prompts = list(prompt)
        else:
            raise ValueError(f"`prompt` has to be a `str` or a non-empty `list` but is {type(prompt)}")
        groups = [prompts]
        if do_classifier_free_guidance:
            if negative_prompt is None:
                negatives = [""] * len(prompts)
            elif isinstance(negative_prompt, str):
                negatives = [negative_prompt] * len(prompts)
            elif len(negative_prompt) != len(prompts):
                raise ValueError(f"`negative_prompt`: {negative_prompt} has batch size {len(negative_prompt)}, but `prompt`: {prompt} has "
                                 f"batch size {len(prompts)}.")
            else:
                negatives = list(negative_prompt)
            groups.append(negatives)
        dtype = self.text_encoder.dtype if self.text_encoder is not None else f16
        out = self._encode_weighted_texts(groups, clip_skip).to(device=device, dtype=dtype)
        b = len(prompts)
        rep = lambda t: t.repeat(1, num_videos_per_prompt, 1).view(b * num_videos_per_prompt, t.shape[1], -1)
        return rep(out[:b]), (rep(out[b:]) if do_classifier_free_guidance else None)

    def enable_vae_slicing(self):
        """pipe:122-128: decode the frames one at a time (peak activation memory / num_frames)."""
        self._vae_slicing = True

    def disable_vae_slicing(self):
        self._vae_slicing = False

    def enable_vae_tiling(self):
        """pipe:139-147: decode (and encode) images larger than one VAE tile -- `vae.tile_sample_min_size` pixels on a side, 512 for
        the SD VAE -- tile by tile with cross-faded seams (`AutoencoderKL.tiled_decode` / `tiled_encode`): peak VAE memory becomes that
        of one tile, and, as in the reference, the frames differ from the untiled ones (every tile has its own GroupNorm statistics
        and mid-block attention).  Composes with `enable_vae_slicing` (per-frame tiled decode) and reaches the condition image's
        encode."""
        if getattr(self, "vae", None) is None:
            raise ValueError("The pipeline must have a `vae` (AutoencoderKL) for using VAE tiling.")
        self.vae.enable_tiling()

    def disable_vae_tiling(self):
        """pipe:149-153."""
        if getattr(self, "vae", None) is None:
            raise ValueError("The pipeline must have a `vae` (AutoencoderKL) for using VAE tiling.")
        self.vae.disable_tiling()

    def enable_freeu(self, s1: float, s2: float, b1: float, b2: float):
        """pipe:155-176: FreeU (https://arxiv.org/abs/2309.11497) on the UNet's first two up blocks -- s1 / s2 attenuate the low
        frequencies of the skip features of stage 1 / 2, b1 / b2 amplify half of the backbone channels (SD-1.5: 0.9, 0.2, 1.2, 1.4).
        The step stays one captured hipGraph (six i2v_freeu_f16 launches in it)."""
        if getattr(self, "unet", None) is None:
            raise ValueError("The pipeline must have `unet` for using FreeU.")
        self.unet.enable_freeu(s1=s1, s2=s2, b1=b1, b2=b2)

    def disable_freeu(self):
        """pipe:179-181."""
        self.unet.disable_freeu()

    def enable_free_init(self, num_iters: int = 3, use_fast_sampling: bool = False, method: str = "butterworth", order: int = 4,
                         spatial_stop_frequency: float = 0.25, temporal_stop_frequency: float = 0.25):
        """diffusers FreeInitMixin.enable_free_init (FreeInit, https://arxiv.org/abs/2312.07537): every call samples the clip `num_iters`
        times.  Between two rounds the clip as the call would return it is diffused back to the first step's noise level with the
        round-0 noise, and one launch group of `i2v_freeinit_mix` keeps its low frequencies over (frames, height, width) -- a
        "butterworth" (with `order`), "gaussian" or "ideal" low-pass at the two stop frequencies -- and takes the high ones from a fresh
        draw of `generator`.  The rounds replay the ONE captured step a plain call uses (enabling this neither enters the graph key nor
        captures); the mix runs as eager launches between the replays.  `use_fast_sampling` gives round i only
        max(1, int(num_inference_steps / num_iters * (i + 1))) steps: the step tables then change shape from round to round, so every
        round re-captures the step (accepted: the cache holds one shape at a time).  num_iters=1 is a plain call, bit for bit."""
        from .free_init import check_free_init_args
        check_free_init_args(num_iters, method, order, spatial_stop_frequency, temporal_stop_frequency)
        self._free_init = dict(num_iters=int(num_iters), use_fast_sampling=bool(use_fast_sampling), method=method, order=int(order),
                               spatial_stop_frequency=float(spatial_stop_frequency),
                               temporal_stop_frequency=float(temporal_stop_frequency))

    def disable_free_init(self):
        """diffusers FreeInitMixin.disable_free_init: one sampling round per call again"""
        self._free_init = None

    @property
    def free_init_enabled(self):
        return self._free_init is not None

    def enable_hires_fix(self, scale=_UNSET, size=None, strength: float = 0.6, num_inference_steps: Optional[int] = None,
                         upscaler: str = "bicubic-antialiased"):
        """The two-pass "hires fix" of the AnimateDiff / A1111 / ComfyUI front ends: every call samples at its `height` x
        `width` as before -- the size the motion modules were trained at --, then upscales the latents, re-noises them to `strength`
        of the schedule and refines them at the target size: `size` = (height, width), or 8 * round(side * `scale` / 8) per side
        (`scale` 1.5 when neither is passed; passing both, or None for both, is refused).  The second pass is what a call with
        `video_latents=upscale_latents(first pass), strength=strength, num_inference_steps=num_inference_steps or the call's,
        height, width = the target` would do, with the same contexts, scheduler, guidance, control arguments and generator objects,
        which go on from where the first pass left them: a `condition_image` is encoded again at the target size, condition latents
        that were passed in are upscaled, control frames and the mask are prepared again.  Its initial latents are ONE launch of
        `i2v_resize_renoise_f32` (upscale and add_noise fused).  `upscaler`: A1111's latent upscalers -- "nearest", "nearest-exact",
        "bilinear", "bicubic", "bilinear-antialiased", "bicubic-antialiased" (torch.nn.functional.interpolate's modes); pixel-space
        upscalers and ESRGAN-class networks are not implemented, and neither is downscaling.  The two sizes are two captured steps:
        while the fix is enabled the graph cache keeps two (both workspaces stay allocated).  FreeInit's rounds belong to the first
        pass.  The defaults are the front ends' usual ones and are unmeasured for quality here."""
        from .hires_fix import DEFAULT_SCALE, check_hires_fix_args
        if scale is _UNSET:
            scale = DEFAULT_SCALE if size is None else None
        self._hires_fix = check_hires_fix_args(scale, size, strength, num_inference_steps, upscaler)

    def disable_hires_fix(self):
        """one pass per call again: every path is what it was before `enable_hires_fix`"""
        self._hires_fix = None

    @property
    def hires_fix_enabled(self):
        return self._hires_fix is not None

    def upscale_latents(self, latents, height, width, upscaler=None):
        """latents fp32 [B, F, C, h, w] -> fp32 [B, F, C, height / 8, width / 8] on the UNet's device: the hires fix's latent upscale
        (`K.resize_renoise` with a = 1 and no noise).  `upscaler`: one of `hires_fix.UPSCALERS`; None takes the enabled fix's, or
        "bicubic-antialiased".  Upscaling only."""
        from .hires_fix import UPSCALERS, device_tables
        if upscaler is None:
            upscaler = self._hires_fix.upscaler if self._hires_fix is not None else "bicubic-antialiased"
        if upscaler not in UPSCALERS:
            raise ValueError(f"unknown upscaler {upscaler!r}: one of {', '.join(UPSCALERS)}")
        if not isinstance(latents, torch.Tensor) or latents.dim() != 5:
            raise ValueError("`latents` must be a [B, F, C, h, w] tensor, got "
                             f"{tuple(latents.shape) if isinstance(latents, torch.Tensor) else type(latents)}")
        if height % self.vae_scale_factor or width % self.vae_scale_factor:
            raise ValueError(f"`height` and `width` have to be divisible by {self.vae_scale_factor} but are {height} and {width}.")
        h, w = latents.shape[-2:]
        h2, w2 = height // self.vae_scale_factor, width // self.vae_scale_factor
        if h2 < h or w2 < w:
            raise ValueError(f"upscale_latents: {h} x {w} -> {h2} x {w2} latents is a downscale, which is not supported")
        if self.unet.device.type != "cuda":
            raise HipLibraryError(f"unet is on {self.unet.device}: the HIP path has no CPU fallback")
        src = latents.detach().to(self.unet.device, torch.float32).contiguous()
        return K.resize_renoise(src, device_tables(h, w, h2, w2, upscaler, src.device))

    def enable_upscaler(self, model_or_path, frames_per_batch: Optional[int] = None, act_type: Optional[str] = None):
        """The pixel-space upscale the AnimateDiff front ends run after sampling: while enabled, the decoded frames of
        every call go through a Real-ESRGAN model -- a compact one (`upscaler.SRVGGNetCompact`: realesr-animevideov3,
        realesr-general-x4v3) or an RRDBNet (`upscaler.RRDBNet`: RealESRGAN_x4plus, RealESRGAN_x4plus_anime_6B), picked by
        the file's keys (`upscaler.load_upscaler`) -- before `tensor2vid` / "pt": s x the size, s the model's `upscale`.
        `model_or_path`: a `SRVGGNetCompact`, an `RRDBNet`, a released `.pth`, a `.safetensors` file or a state dict (`act_type` "relu" /
        "leakyrelu" for a compact dict without PReLU weights; with an RRDBNet it is a ValueError).  `frames_per_batch`
        frames go through the network at a time (None: all of them; one under `enable_vae_slicing`): frames are independent, so the
        result is the same bits for every chunking.  There is nothing to upscale in latents: a call with output_type="latent" is
        refused while the upscaler is enabled.  The sampler and the captured step are untouched.
        Memory of an RRDBNet: three dense-block buffers of 192 channels at the input size plus two 64-channel activations at 4 x the
        size are alive at the peak -- for 16 frames of 512 x 512, 3 x 1.6 GB = 4.8 GB and 2 x 8.6 GB at 2048 x 2048 (fp16), next to the
        fp32 result (3.2 GB).  `frames_per_batch` bounds it: the peak is per chunk."""
        from .upscaler import RRDBNet, SRVGGNetCompact, load_upscaler
        if frames_per_batch is not None and (isinstance(frames_per_batch, bool) or not isinstance(frames_per_batch, int)
                                             or frames_per_batch < 1):
            raise ValueError(f"`frames_per_batch` must be a positive integer or None, got {frames_per_batch!r}")
        if isinstance(model_or_path, SRVGGNetCompact):
            if act_type is not None and act_type != model_or_path.act_type:
                raise ValueError(f"act_type={act_type!r}, but the model was built with {model_or_path.act_type!r}")
            model = model_or_path
        elif isinstance(model_or_path, RRDBNet):
            if act_type is not None:
                raise ValueError(f"act_type={act_type!r} with an RRDBNet: the architecture's activation is LeakyReLU(0.2)")
            model = model_or_path
        else:
            model = load_upscaler(model_or_path, act_type=act_type)
            unet = getattr(self, "unet", None)
            if unet is not None and unet.device.type == "cuda":
                model = model.to(unet.device)
        self._upscaler = (model, frames_per_batch)

    def disable_upscaler(self):
        """the decoded frames are the output again: every path is what it was before `enable_upscaler`"""
        self._upscaler = None

    @property
    def upscaler_enabled(self):
        return self._upscaler is not None

    def upscale_frames(self, video):
        """video [B, F, 3, H, W] or [N, 3, H, W] in [-1, 1] (`decode_latents`' result) -> fp32 of the same rank at s x the size, in
        [-1, 1], through the enabled upscaler, `frames_per_batch` frames (one under `enable_vae_slicing`) at a time."""
        if self._upscaler is None:
            raise ValueError("upscale_frames needs an upscaler: enable_upscaler(model_or_path) first")
        model, per = self._upscaler
        if not isinstance(video, torch.Tensor) or video.dim() not in (4, 5) or video.shape[-3] != 3:
            raise ValueError("`video` must be a [B, F, 3, H, W] or [N, 3, H, W] tensor, got "
                             f"{tuple(video.shape) if isinstance(video, torch.Tensor) else type(video)}")
        if model.device.type != "cuda":
            raise HipLibraryError(f"the upscaler is on {model.device}: the HIP path has no CPU fallback")
        flat = video.detach().to(model.device).reshape((-1,) + tuple(video.shape[-3:]))
        n = flat.shape[0]
        per = 1 if self._vae_slicing else (per or n)
        out = torch.cat([model(flat[i: i + per], signed=True) for i in range(0, n, per)])
        return out.reshape(tuple(video.shape[:-2]) + tuple(out.shape[-2:]))

    def enable_free_noise(self, context_length: int = 16, context_stride: int = 4, weighting_scheme: str = "pyramid",
                          noise_type: str = "shuffle_context"):
        """diffusers AnimateDiffFreeNoiseMixin.enable_free_noise (FreeNoise, https://arxiv.org/abs/2310.15169): clips longer than the
        motion modules' positional table (`num_frames` 32, 64, 128 from a 16-frame motion adapter).  The motion modules attend inside
        sliding windows of `context_length` frames, `context_stride` apart, and average the windows per frame (`weighting_scheme`:
        "flat", "pyramid", "delayed_reverse_sawtooth"); the initial noise of the frames behind the first window is a reshuffle of
        the first window's (`noise_type`: "shuffle_context", "repeat_context", "random").  The step stays one captured hipGraph,
        re-captured once when the settings change."""
        if getattr(self, "unet", None) is None:
            raise ValueError("The pipeline must have `unet` for using FreeNoise.")
        self.unet.enable_free_noise(context_length=context_length, context_stride=context_stride, weighting_scheme=weighting_scheme,
                                    noise_type=noise_type)

    def disable_free_noise(self):
        """diffusers disable_free_noise"""
        self.unet.disable_free_noise()

    def _free_noise_settings(self):
        """the UNet's `free_noise.FreeNoiseSettings`, or None while FreeNoise is off"""
        sig = self.unet.free_noise_signature()
        if sig is None:
            return None
        from .free_noise import FreeNoiseSettings
        return FreeNoiseSettings(*sig)

    @property
    def free_noise_enabled(self):
        return self.unet.free_noise_signature() is not None

    def decode_latents(self, latents):
        """pipe:300-320: latents (B, F, 4, h, w) -> video (B, F, 3, 8h, 8w) float32 through the HIP VAE decoder."""
        if self.vae is None:
            raise ValueError("decode_latents needs a `vae` (AutoencoderKL or AutoencoderTiny) -- or use output_type='latent'")
        latents = 1 / self.vae.config["scaling_factor"] * latents
        b, f, c, h, w = latents.shape
        flat = latents.reshape(b * f, c, h, w)
        if self._vae_slicing:
            image = torch.cat([self.vae.decode(flat[i: i + 1]).sample for i in range(b * f)])
        else:
            image = self.vae.decode(flat).sample
        return image[None, :].reshape((b, f, -1) + image.shape[2:]).float()

    def encode_condition_image(self, condition_image, height, width, generator=None):
        """pipe:626-627: preprocess -> vae.encode(...).latent_dist.sample() * scaling_factor.  A deterministic VAE (AutoencoderTiny:
        the result of `encode` has `latents` and no `latent_dist`) gives its latents as they are: nothing is sampled and `generator`
        is not used."""
        if self.vae is None:
            raise ValueError("a `condition_image` needs a `vae` (AutoencoderKL) -- or pass `condition_image_latents`")
        img = self.image_processor.preprocess(condition_image, height=height, width=width).to(self.vae.device)
        if isinstance(generator, list):
            generator = generator[0]
        enc = self.vae.encode(img)
        if not hasattr(enc, "latent_dist") and hasattr(enc, "latents"):
            return enc.latents * self.vae.config["scaling_factor"]
        return enc.latent_dist.sample(generator) * self.vae.config["scaling_factor"]

    def to(self, device=None, dtype=None):
        """move the models the pipeline holds (pipe:784); fp16 is the storage dtype of the HIP path."""
        for name in ("unet", "vae", "text_encoder", "image_encoder", "controlnet", "t2i_adapter"):
            m = getattr(self, name)
            if m is not None:
                setattr(self, name, m.to(device=device, dtype=dtype))
        return self

    def load_i2v_adapter(self, i2v_adapter):
        self.unet.load_i2v_adapter(i2v_adapter)
        self.i2v_adapter = i2v_adapter

    def load_ip_adapter(self, pretrained_model_name_or_path_or_dict, subfolder: Optional[str] = None,
                        weight_name: Optional[str] = None, **_unused):
        """diffusers IPAdapterMixin.load_ip_adapter as called at pipe:783: reads ip-adapter_sd15.{bin,safetensors} or an IP-Adapter Plus
        file (ip-adapter-plus_sd15, ip-adapter-plus-face_sd15) and installs the decoupled cross-attention branch + ImageProjection, or
        + Resampler for Plus (unet:1230-1287; Full Face raises).  As diffusers does, a pipeline without an
        `image_encoder` takes it from `<path>/<subfolder>/image_encoder` when the argument is a path and that folder exists (the HIP
        `CLIPVisionModelWithProjection`, moved to the UNet's device and dtype; no folder: `image_encoder` stays None and only
        `image_embeds` can be passed), and a pipeline without a `feature_extractor` gets transformers' `CLIPImageProcessor()` when
        transformers is importable (any object with that call interface works)."""
        from .checkpoint import load_ip_adapter_file
        self.unet._load_ip_adapter_weights(
            load_ip_adapter_file(pretrained_model_name_or_path_or_dict, subfolder=subfolder, weight_name=weight_name),
            num_image_tokens=self._image_encoder_tokens())
        if self.image_encoder is None and not isinstance(pretrained_model_name_or_path_or_dict, dict):
            folder = os.path.join(pretrained_model_name_or_path_or_dict, subfolder or "", "image_encoder")
            if os.path.isdir(folder):
                from .clip_vision import CLIPVisionModelWithProjection
                logger.info(f"loading image_encoder from {folder}")
                enc = CLIPVisionModelWithProjection.from_pretrained(folder)
                self.image_encoder = enc.to(device=self.unet.device, dtype=self.unet.dtype)
                if isinstance(self.unet.encoder_hid_proj, Resampler):
                    self.unet.encoder_hid_proj.check_tokens(self._image_encoder_tokens())
        if self.feature_extractor is None:
            try:
                from transformers import CLIPImageProcessor
                self.feature_extractor = CLIPImageProcessor()
            except ImportError:
                pass

    def _image_encoder_tokens(self):
        """tokens per image of `image_encoder`'s hidden states (what a Resampler attends to), None without an encoder"""
        cfg = getattr(self.image_encoder, "config", None)
        if cfg is None or getattr(cfg, "image_size", None) is None or getattr(cfg, "patch_size", None) is None:
            return None
        return (cfg.image_size // cfg.patch_size) ** 2 + 1

    def set_ip_adapter_scale(self, scale: float):
        """diffusers IPAdapterMixin.set_ip_adapter_scale: the weight of the image-prompt branch in every cross-attention that carries
        one.  The scale is a launch argument of the captured step, so the next call re-captures once (`_graph_key` holds it)."""
        for attn in self.unet._cross_attention_layers():
            if attn.ip_num_tokens:
                attn.ip_scale = float(scale)

    # ------------------------------------------------------------------------------------------ LoRA (lora.py)
    def load_lora_weights(self, pretrained_model_name_or_path_or_dict, adapter_name: Optional[str] = None,
                          weight_name: Optional[str] = None, subfolder: Optional[str] = None):
        """diffusers LoraLoaderMixin.load_lora_weights (pipe:57): a .safetensors / .bin file or a state dict in the diffusers, PEFT or
        kohya key spelling; the UNet part is kept as a named adapter and MERGED into the UNet's weights at the next call (one
        i2v_lora_merge launch per targeted weight, nothing per denoising step).  Text-encoder keys are skipped (CLIP is out of scope) and
        counted in the returned report."""
        return self.unet.load_lora(pretrained_model_name_or_path_or_dict, adapter_name=adapter_name, weight_name=weight_name,
                                   subfolder=subfolder)

    def set_adapters(self, adapter_names, adapter_weights=None):
        self.unet.set_adapters(adapter_names, adapter_weights)

    def get_active_adapters(self):
        return self.unet.get_active_adapters()

    def delete_adapters(self, adapter_names):
        self.unet.delete_adapters(adapter_names)

    def unload_lora_weights(self):
        """the UNet's weights get their values from before the first load back, bit for bit"""
        self.unet.unload_lora()

    def fuse_lora(self, lora_scale: float = 1.0):
        """merge the active adapters at `lora_scale` now and drop their factors (the per-call scale no longer applies)"""
        self.unet.fuse_lora(lora_scale)

    def unfuse_lora(self):
        """the weights from before the LoRA, exactly (restored from the stash, not by subtracting the update as diffusers does)"""
        self.unet.unfuse_lora()

    def load_motion_adapter(self, motion_adapter):
        self.unet.load_motion_modules(motion_adapter)
        self.motion_adapter = motion_adapter

    def get_timesteps(self, num_inference_steps, strength, device=None):
        """pipe:529-536."""
        init_timestep = min(int(num_inference_steps * strength), num_inference_steps)
        t_start = max(num_inference_steps - init_timestep, 0)
        return self.scheduler.timesteps[t_start:], num_inference_steps - t_start

    def prepare_latents(self, batch_size, num_channels_latents, num_frames, height, width, dtype, device,
                        generator, latents=None):
        """pipe:265-297 (noise drawn on the host generator so that a seed reproduces the CPU oracle's draw)."""
        shape = (batch_size, num_frames, num_channels_latents, height // self.vae_scale_factor,
                 width // self.vae_scale_factor)
        if isinstance(generator, list) and len(generator) != batch_size:
            raise ValueError(
                f"You have passed a list of generators of length {len(generator)}, but requested an effective batch"
                f" size of {batch_size}. Make sure the batch size matches the length of the generators.")
        if latents is None:
            if isinstance(generator, list):                                   # one generator per sample (pipe:287-290)
                latents = torch.cat([_draw(torch.randn, (1,) + shape[1:], g, device) for g in generator], dim=0)
            else:
                latents = _draw(torch.randn, shape, generator, device)
        return latents.to(device=device, dtype=torch.float32) * self.scheduler.init_noise_sigma

    # ------------------------------------------------------------------------------------------ one step
    def _scheduler_kind(self):
        """"dpmsolver++" for a DPMSolverMultistepScheduler (the i2v_dpm_cfg_step update), "lcm" for an LCMScheduler (the
        i2v_lcm_cfg_step update), "euler" / "euler_ancestral" for this package's EulerDiscreteScheduler / EulerAncestralDiscreteScheduler
        (i2v_sigma_prep and the i2v_euler_cfg_step update), "ddim" for any other scheduler object (the DDIM update, as before); the
        reference's other schedulers by class name raise -- a foreign object named like one of the Euler classes too."""
        if isinstance(self.scheduler, EulerAncestralDiscreteScheduler):
            return "euler_ancestral"
        if isinstance(self.scheduler, EulerDiscreteScheduler):
            return "euler"
        if isinstance(self.scheduler, LCMScheduler):
            return "lcm"
        if isinstance(self.scheduler, DPMSolverMultistepScheduler):
            return "dpmsolver++"
        name = type(self.scheduler).__name__
        if name in UNSUPPORTED_SCHEDULERS:
            raise NotImplementedError(f"{name} is not supported by this build: use DDIMScheduler or DPMSolverMultistepScheduler "
                                      "(e.g. DPMSolverMultistepScheduler.from_config(pipe.scheduler.config)), or LCMScheduler with an "
                                      "LCM-LoRA; Euler and Euler-ancestral sampling run with this package's own EulerDiscreteScheduler / "
                                      "EulerAncestralDiscreteScheduler (e.g. EulerDiscreteScheduler.from_config(pipe.scheduler.config))")
        return "ddim"

    def _step(self, st):
        """One iteration of pipe:666-697 as kernel launches on the current stream (captured into a hipGraph)."""
        unet = self.unet
        sigma_space = isinstance(self.scheduler, (EulerDiscreteScheduler, EulerAncestralDiscreteScheduler))
        if sigma_space:
            # scale_model_input: the model input is the latents / sqrt(sigma^2 + 1), frame 0 included; the latents keep the bare condition
            x = K.sigma_prep(st["latents"], st["cond"], st["coef"], st["step_idx"], unet.packed()["cin_pad"], st["copies"])
        else:
            x = K.ddim_prep(st["latents"], st["cond"], unet.packed()["cin_pad"], st["copies"])  # pipe:668-673
        # the time-embedding chain of this step's timestep: one row of the table computed once per sample (_time_table)
        temb_proj = K.select_row(st["temb_table"], st["step_idx"])
        control = {}
        if isinstance(st.get("cn_cond"), tuple):
            # several ControlNets: one after the other on this stream (no parallel branches in the captured graph), each on the step's
            # model input with its own control frames, context projection and time table; the UNet adds all their residuals in one
            # launch per add, each net at this step's value of its own row of the [N, steps] scale table
            sets = [net._fwd_tokens(x, K.select_row(temb, st["step_idx"]), ctx, cond) for net, temb, ctx, cond in
                    zip(self.controlnet.nets, st["cn_temb_table"], st["cn_ctx_proj"], st["cn_cond"])]
            control = dict(residual_sets=sets, residual_scale=(st["cn_scale"], st["step_idx"]))
        elif st.get("cn_cond") is not None:
            # the ControlNet reads the step's model input -- frame 0 already replaced by the condition latents, the tensor the UNet
            # reads -- and writes its 12 + 1 residuals; the UNet adds them at this step's row of the scale table
            down, mid = self.controlnet._fwd_tokens(x, K.select_row(st["cn_temb_table"], st["step_idx"]), st["cn_ctx_proj"], st["cn_cond"])
            control = dict(down_residuals=down, mid_residual=mid, residual_scale=(st["cn_scale"], st["step_idx"]))
        if st.get("t2i_feats") is not None:
            # the T2I-Adapter's four feature maps were computed once per sample: the step only adds them, at this step's row of the
            # adapter's scale table (one copy of the features serves both CFG halves)
            control.update(intrablock_residuals=st["t2i_feats"], intrablock_scale=(st["t2i_scale"], st["step_idx"]))
        # the CFG halves are copies of one tensor at one timestep (pipe:672-673): what does not depend on the prompt is
        # computed once (unet._fwd_tokens, cfg_shared)
        y = unet._fwd_tokens(x, None, True, st.get("ctx_proj") or st["ctx_text"], st["ctx_ip"],
                             st["num_frames"], cfg_shared=CFG_SHARED and st["copies"] == 2, temb_proj=temb_proj,
                             forward_upsample_size=any(s % (2 ** unet.num_upsamplers) for s in st["latents"].shape[-2:]),
                             **control)                                                          # pipe:676-683, unet:1304-1311
        if sigma_space:
            K.euler_cfg_step(st["latents"], st.get("noise"), y, st["coef"], st["step_idx"], st["guidance"], st["copies"])
        elif isinstance(self.scheduler, LCMScheduler):
            K.lcm_cfg_step(st["latents"], st["noise"], y, st["coef"], st["step_idx"], st["guidance"], st["copies"])
        elif isinstance(self.scheduler, DPMSolverMultistepScheduler):
            K.dpm_cfg_step(st["latents"], st["x0_prev"], y, st["coef"], st["step_idx"], st["guidance"], st["copies"])
        else:
            K.ddim_cfg_step(st["latents"], y, st["coef"], st["step_idx"], st["guidance"], st["copies"])  # pipe:686-691
        if st.get("v2v_mask") is not None:
            # video-to-video with a mask: the same launch under every scheduler.  The scheduler step has advanced the counter (and
            # wrapped it after the last step), so the launch reads the row of the NEXT timestep -- row 0, the clean source, at the end
            K.masked_renoise(st["latents"], st["v2v_source"], st["v2v_noise"], st["v2v_mask"], st["v2v_coef"], st["step_idx"])

    def _project_once(self, st, into=False):
        """what depends on the sample but not on the step, computed once before the steps: K / V^T of the context for every
        cross-attention layer and the time-embedding chain of the whole schedule -- the UNet's and, with a ControlNet, the ControlNet's
        own.  into: overwrite the buffers `st` already holds (a cached graph's static buffers)."""
        old = (lambda name: st[name]) if into else (lambda name: None)
        st["ctx_proj"] = self.unet.project_context(st["ctx_text"], st["ctx_ip"], out=old("ctx_proj"))
        st["temb_table"] = self.unet.project_time_table(st["t_table"], out=old("temb_table"))
        if isinstance(st.get("cn_cond"), tuple):                      # several ControlNets: one projection and one table per net
            nets = self.controlnet.nets
            olds = lambda name: old(name) or (None,) * len(nets)
            st["cn_ctx_proj"] = tuple(net.project_context(st["ctx_text"], out=o) for net, o in zip(nets, olds("cn_ctx_proj")))
            st["cn_temb_table"] = tuple(net.project_time_table(st["t_table"], out=o) for net, o in zip(nets, olds("cn_temb_table")))
        elif st.get("cn_cond") is not None:
            st["cn_ctx_proj"] = self.controlnet.project_context(st["ctx_text"], out=old("cn_ctx_proj"))
            st["cn_temb_table"] = self.controlnet.project_time_table(st["t_table"], out=old("cn_temb_table"))

    def _graph_key(self, st):
        """everything a captured step has baked in besides the contents of the static buffers: shapes, the Python
        scalars passed as launch arguments (guidance, IP scales), the identity / version of every weight (the packed
        kernel-layout copies are rebuilt when a parameter changes, and a graph captured before that reads the old ones) and the
        scheduler's update (a scheduler swapped between calls re-captures) and FreeU's four scales (launch arguments: enabling,
        changing or disabling FreeU re-captures) and the LCM noise table's shape (its row count is a launch argument: another step
        count re-captures) and FreeNoise's window settings (they decide the launches of every motion module: enabling, changing or
        disabling FreeNoise re-captures; its noise_type only shapes the initial noise and does not).  The shapes and dtypes are those
        of SAMPLE_INPUTS, all of them: which of the optional ones are present says which launches the step has (a ControlNet's, a
        T2I-Adapter's adds, a mask's blend -- a source clip without a mask launches nothing of its own and leaves no entry: its key is
        a plain call's), and the tables' row counts are launch arguments.  With a ControlNet, its weights as the UNet's."""
        unet = self.unet
        wsig = hash(tuple((p.data_ptr(), p._version) for p in unet.parameters()))
        cn_wsig = hash(self.controlnet.weight_signature()) if st.get("cn_cond") is not None else None
        ips = tuple((a.ip_num_tokens, float(a.ip_scale)) for a in unet._cross_attention_layers())
        # (a captured step keeps the residual-stream mode it was captured in)
        return (cn_wsig, st["copies"], st["num_frames"], st["guidance"], str(st["latents"].device), wsig, ips, blocks.precise_stream(),
                self._scheduler_kind(), unet.freeu_signature(), unet.free_noise_launch_signature()) + _sample_input_shapes(st)

    def _run_steps(self, st, n_steps, use_graph):
        if not use_graph:
            self._project_once(st)
            for _ in range(n_steps):
                self._step(st)
            return st["latents"]
        # The captured step is kept across calls: a second sample of the same shape (the evaluation driver's loop) copies
        # its inputs into the graph's static buffers and replays -- no eager warm-up step, no re-capture (~0.3 s of a
        # 1.8 s sample at 16 f x 512 x 512).
        key = self._graph_key(st)
        cache = self._graph_cache
        hit = cache.get(key)
        if hit is not None:
            graph, gst = hit
            cache[key] = cache.pop(key)     # (most recently used last)
            _copy_sample_inputs(gst, st)
            self._project_once(gst, into=True)
        else:
            # one shape at a time (a graph pins its workspace): the old graph and its pool go before the new capture,
            # so two pools never coexist at the peak.  While the hires fix is enabled, two: its passes have one size each, and the
            # most recently used graph stays beside the new one
            keep = 1 if self._hires_fix is not None else 0
            for old in list(cache)[:max(len(cache) - keep, 0)]:
                del cache[old]
            self._graph = None
            self._project_once(st)
            # warm-up outside capture: packs weights, sizes the allocator; then restore the state it advanced
            saved = st["latents"].clone()
            self._step(st)
            st["latents"].copy_(saved)
            st["step_idx"].zero_()
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                self._step(st)
            st["latents"].copy_(saved)      # capture does not execute, but keep the invariant explicit
            st["step_idx"].zero_()
            gst = dict(st)                  # its own dict: the caller goes on to rebind entries of `st`
            cache[key] = (graph, gst)
        self._graph = graph
        for _ in range(n_steps):
            graph.replay()
        return gst["latents"].clone()     # the static buffer stays with the graph; the caller gets its own tensor

    def _resolve_call_defaults(self, output_type, callback, use_graph):
        """(output_type, use_graph) as `__call__` uses them.  output_type=None is the reference's default "pil" (pipe:556);
        a pipeline assembled without a VAE (latents in, latents out: the benchmarks and most tests) has nothing to decode
        with and returns the latents.  pipe:693-697 calls back after every step: a replayed hipGraph has no per-step host
        hook, so a `callback` runs the same kernels as eager launches (bit-identical, tests/test_modules_gpu.py)."""
        if output_type is None:
            output_type = "pil" if self.vae is not None else "latent"
        if callback is not None:
            use_graph = False
        return output_type, use_graph

    # ------------------------------------------------------------------------------------------ ControlNet
    def _check_control_args(self, control_image, num_frames, scale, start, end, guess_mode):
        """the ControlNet arguments of a call, checked on the host before anything is launched or encoded"""
        if guess_mode:
            raise NotImplementedError("guess_mode=True is not implemented")
        if control_image is not None and self.controlnet is None:
            raise ValueError("`control_image` was passed but the pipeline has no `controlnet`: build it with "
                             "I2VAdapterPipeline(..., controlnet=ControlNetModel.from_pretrained(...))")
        if self.controlnet is None:
            return
        if control_image is None:
            raise ValueError("the pipeline has a `controlnet`: `control_image` is required (one control frame per frame of the clip)")
        from .controlnet import controlnet_keep_table
        if self._multi_controlnet():
            nets = self.controlnet.nets
            if not isinstance(control_image, (list, tuple)) or len(control_image) != len(nets):
                n = len(control_image) if isinstance(control_image, (list, tuple)) else 1
                raise ValueError(f"`control_image` holds {n} entries, the pipeline has {len(nets)} ControlNets: with a "
                                 "MultiControlNetModel it is a list with one entry per net, each what a single ControlNet takes")
            for k, (net, frames, args) in enumerate(zip(nets, control_image, self._control_args(scale, start, end))):
                controlnet_keep_table(1, *args)                        # each net's own window
                n = _frame_count(frames, f"control_image[{k}]", net.config.conditioning_channels, "the ControlNet's `conditioning_channels`")
                if n != num_frames:
                    raise ValueError(f"`control_image[{k}]` holds {n} frames, `num_frames` is {num_frames}: a ControlNet runs per frame "
                                     "and needs one control frame for every frame of the clip")
            return
        controlnet_keep_table(1, scale, start, end)                    # 0 <= start < end <= 1, else ValueError
        n = _frame_count(control_image, "control_image", 3)
        if n != num_frames:
            raise ValueError(f"`control_image` holds {n} frames, `num_frames` is {num_frames}: a ControlNet runs per frame and needs one "
                             "control frame for every frame of the clip")

    def prepare_control_image(self, control_image, batch_size, num_frames, height, width, channels: int = 3):
        """-> fp32 [batch_size * num_frames, 3, height, width] in [0, 1] on the host: PIL images resized by the image processor WITHOUT
        the [-1, 1] normalisation (a ControlNet is trained on [0, 1] maps); tensors as they are (they must have that size); one clip
        of control frames is shared by the batch.  channels: a net's `conditioning_channels` where it is not 3 (a net of a
        MultiControlNetModel) -- tensors must have that many, PIL images are converted to "L" for 1."""
        if isinstance(control_image, torch.Tensor):
            t = _frame_tensor(control_image, "control_image", height, width, batch_size, num_frames,
                              *(() if channels == 3 else (channels, "the ControlNet's `conditioning_channels`")))
        else:
            if len(control_image) != num_frames:
                raise ValueError(f"`control_image` holds {len(control_image)} frames, `num_frames` is {num_frames}")
            if channels == 1:
                t = torch.stack([_pil_plane(im, "control_image", "L", height, width)[None] for im in control_image])
            else:
                t = self.control_image_processor.preprocess(list(control_image), height=height, width=width)
            if tuple(t.shape[-2:]) != (height, width):
                raise ValueError(f"control frames of {tuple(t.shape[-2:])} after resizing, expected {height} x {width}")
            t = t[None].expand(batch_size, -1, -1, -1, -1)
        return t.reshape(batch_size * num_frames, channels, height, width).contiguous()

    def _multi_controlnet(self):
        from .controlnet import MultiControlNetModel
        return isinstance(self.controlnet, MultiControlNetModel)

    def _control_args(self, scale, start, end):
        """(scale, start, end) of a call as `_schedule_tables` keeps them: three floats, or with a MultiControlNetModel one such triple
        per net -- each argument a number for all nets or a list with one entry per net (diffusers' rule); a list of another length
        is a ValueError."""
        if not self._multi_controlnet():
            return float(scale), float(start), float(end)
        n = len(self.controlnet.nets)
        cols = []
        for name, v in (("controlnet_conditioning_scale", scale), ("control_guidance_start", start), ("control_guidance_end", end)):
            if isinstance(v, (list, tuple)):
                if len(v) != n:
                    raise ValueError(f"`{name}` holds {len(v)} values, the pipeline has {n} ControlNets: pass one number for all "
                                     "nets or a list with one per net")
                cols.append([float(x) for x in v])
            else:
                cols.append([float(v)] * n)
        return tuple(zip(*cols))

    # ------------------------------------------------------------------------------------------ T2I-Adapter
    def _check_adapter_args(self, adapter_image, num_frames, scale, factor):
        """the T2I-Adapter arguments of a call, checked on the host before anything is launched or encoded"""
        if adapter_image is not None and self.t2i_adapter is None:
            raise ValueError("`adapter_image` was passed but the pipeline has no `t2i_adapter`: build it with "
                             "I2VAdapterPipeline(..., t2i_adapter=T2IAdapter.from_pretrained(...))")
        if self.t2i_adapter is None:
            return
        if adapter_image is None:
            raise ValueError("the pipeline has a `t2i_adapter`: `adapter_image` is required (one control frame per frame of the clip)")
        from .t2i_adapter import adapter_scale_table
        adapter_scale_table(1, scale, factor)                          # 0 <= factor <= 1, else ValueError
        n = _frame_count(adapter_image, "adapter_image", self.t2i_adapter.config.in_channels, "the adapter's `in_channels`")
        if n != num_frames:
            raise ValueError(f"`adapter_image` holds {n} frames, `num_frames` is {num_frames}: a T2I-Adapter runs per frame and needs one "
                             "control frame for every frame of the clip")

    def prepare_adapter_image(self, adapter_image, batch_size, num_frames, height, width):
        """-> fp32 [batch_size * num_frames, in_channels, height, width] in [0, 1] on the host, like `prepare_control_image` (no
        [-1, 1] normalisation): PIL images are converted to "L" for a 1-channel adapter (canny, sketch) and to "RGB" for a 3-channel
        one and resized; tensors are taken as they are (they must have that size); one clip of frames is shared by the batch."""
        c = self.t2i_adapter.config.in_channels
        if isinstance(adapter_image, torch.Tensor):
            t = _frame_tensor(adapter_image, "adapter_image", height, width, batch_size, num_frames, c, "the adapter's `in_channels`")
        else:
            if len(adapter_image) != num_frames:
                raise ValueError(f"`adapter_image` holds {len(adapter_image)} frames, `num_frames` is {num_frames}")
            planes = [_pil_plane(im, "adapter_image", "L" if c == 1 else "RGB", height, width) for im in adapter_image]
            t = torch.stack([p[None] if c == 1 else p.permute(2, 0, 1) for p in planes])[None].expand(batch_size, -1, -1, -1, -1)
        return t.reshape(batch_size * num_frames, c, height, width).contiguous()

    # ------------------------------------------------------------------------------------------ video-to-video, masked editing
    def _check_video_args(self, video, video_latents, strength, mask_image, num_frames, num_inference_steps, ratio, eta):
        """the video-to-video arguments of a call, checked on the host before anything is launched or encoded.  Returns (video,
        video_latents, strength): the source clip cut to `num_frames` frames and the strength with its default (0.8 with a clip)."""
        if video is not None and video_latents is not None:
            raise ValueError("Cannot forward both `video` and `video_latents`. Please make sure to only forward one of the two.")
        if video is None and video_latents is None:
            if strength is not None:
                raise ValueError(f"`strength` = {strength} was passed without a source clip: it is the fraction of the schedule a `video` "
                                 "(or `video_latents`) is noised to")
            if mask_image is not None:
                raise ValueError("`mask_image` was passed without a source clip: it needs `video` (or `video_latents`), the clip whose "
                                 "region outside the mask is kept")
            return None, None, None
        if video is not None:
            n = _frame_count(video, "video", 3)
        else:
            if not isinstance(video_latents, torch.Tensor) or video_latents.dim() != 5:
                raise ValueError("`video_latents` must be a [B, F, 4, h, w] tensor, got "
                                 f"{tuple(video_latents.shape) if isinstance(video_latents, torch.Tensor) else type(video_latents)}")
            n = video_latents.shape[1]
        if n < num_frames:
            raise ValueError(f"the source clip holds {n} frames, `num_frames` is {num_frames}: video-to-video needs one source frame for "
                             "every frame of the clip")
        if video_latents is not None:
            video_latents = video_latents[:, :num_frames]
        elif isinstance(video, torch.Tensor):
            video = video[..., :num_frames, :, :, :]
        else:
            video = list(video[:num_frames])
        strength = 0.8 if strength is None else float(strength)
        if not 0.0 < strength <= 1.0:
            raise ValueError(f"The value of strength should in (0.0, 1.0] but is {strength}")
        steps = min(int(num_inference_steps * strength), num_inference_steps)
        if steps < 1:
            raise ValueError(f"After adjusting the num_inference_steps by strength parameter: {strength}, the number of pipeline "
                             f"steps is {steps} which is < 1 and not appropriate for this pipeline.")
        if ratio != 1:
            raise ValueError(f"`frame_similarity_sample_ratio` = {ratio} with a source clip: `strength` decides where the schedule "
                             "starts, leave the ratio at 1")
        if self._free_init is not None:
            raise ValueError("a source clip (`video` / `video_latents`) while FreeInit is enabled is not supported: "
                             "disable_free_init() first")
        if mask_image is not None and eta > 0 and self._scheduler_kind() == "ddim":
            raise ValueError(f"`mask_image` with eta = {eta} > 0: the stochastic DDIM update adds its noise after the mask's blend and "
                             "would noise the kept region -- use eta = 0")
        if video is not None and self.vae is None:
            raise ValueError("a `video` needs a `vae` (AutoencoderKL or AutoencoderTiny) -- or pass `video_latents`")
        return video, video_latents, strength

    def _video_frames(self, video, height, width):
        """-> fp32 [B or 1, F, 3, height, width] in [-1, 1] on the host: PIL frames through `image_processor.preprocess` (resized, as the
        condition image is); tensors in [0, 1] are normalised and must already have that size"""
        if isinstance(video, torch.Tensor):
            _frame_count(video, "video", 3)
            t = _frame_tensor(video, "video", height, width)
            flat = self.image_processor.preprocess(t.reshape(-1, 3, height, width))
            return flat.reshape(t.shape[0], t.shape[1], 3, height, width)
        flat = self.image_processor.preprocess(list(video), height=height, width=width)
        if tuple(flat.shape[-2:]) != (height, width):
            raise ValueError(f"video frames of {tuple(flat.shape[-2:])} after resizing, expected {height} x {width}")
        return flat[None]

    def encode_video(self, video, height, width, generator=None):
        """video (PIL frames, [F, 3, H, W] in [0, 1], or [B, F, 3, H, W]) -> latents [B, F, 4, height / 8, width / 8] fp32, scaled: all
        B * F frames through `vae.encode` (frame by frame under `enable_vae_slicing`; tiled under `enable_vae_tiling`, as the condition
        image is), then ONE draw of `latent_dist.sample` over the [B * F, 4, h, w] moments in (sample, frame) order (a list of generators:
        generator b draws sample b's frames), times `scaling_factor`.  A deterministic VAE (AutoencoderTiny) gives its latents
        undrawn."""
        if self.vae is None:
            raise ValueError("a `video` needs a `vae` (AutoencoderKL or AutoencoderTiny) -- or pass `video_latents`")
        return self._encode_frames(self._video_frames(video, height, width), generator)

    def _encode_frames(self, frames, generator=None):
        """`encode_video` behind the preprocessing: frames fp32 [B, F, 3, H, W] in [-1, 1] on the host"""
        b, f = frames.shape[:2]
        flat = frames.reshape(b * f, *frames.shape[2:]).to(self.vae.device)
        chunks = [flat[i: i + 1] for i in range(b * f)] if self._vae_slicing else [flat]
        encs = [self.vae.encode(c) for c in chunks]
        scale = self.vae.config["scaling_factor"]
        if not hasattr(encs[0], "latent_dist") and hasattr(encs[0], "latents"):
            lat = torch.cat([e.latents for e in encs])
            return (lat * scale).reshape(b, f, *lat.shape[1:])
        moments = torch.cat([e.latent_dist.parameters for e in encs]).contiguous()
        n, c2, h, w = moments.shape
        eps = _draw(torch.randn, (b, f, c2 // 2, h, w), generator, moments.device).reshape(n, c2 // 2, h, w).contiguous()
        return (K.gaussian_sample(moments, eps) * scale).reshape(b, f, c2 // 2, h, w)

    def prepare_video_latents(self, video_latents, noise, timestep):
        """the initial latents of video-to-video: scheduler.add_noise(video_latents, noise, timestep) =
        sqrt(abar_t) * video_latents + sqrt(1 - abar_t) * noise (a sigma-space sampler: video_latents + sigma_t * noise), on a copy of the
        source (fp32 [B, F, 4, h, w] on the device; K.axpby)"""
        sa, sb = self._noise_level(timestep)
        return K.axpby(video_latents.detach().to(torch.float32).clone(memory_format=torch.contiguous_format),
                       noise.to(torch.float32).contiguous(), sa, sb)

    def _noise_level(self, timestep):
        """(a, b) of `add_noise` = a x0 + b noise at `timestep`: (sqrt(abar_t), sqrt(1 - abar_t)) as `add_noise` computes them, in fp32; a
        scheduler with a `noise_level` of its own (the Euler samplers: (1, sigma_t), fractional timesteps) is asked instead"""
        if hasattr(self.scheduler, "noise_level"):
            return self.scheduler.noise_level(timestep)
        a = self.scheduler.alphas_cumprod[int(timestep)].to(torch.float32)
        return float(a ** 0.5), float((1 - a) ** 0.5)

    def _prior_level(self, timestep):
        """(a, b) the prior and FreeInit's mix noise to: (abar_t^0.5, (1 - abar_t)^0.5) from abar_t as a Python float, as these two
        always computed it; a scheduler with a `noise_level` of its own is asked instead"""
        if hasattr(self.scheduler, "noise_level"):
            return self.scheduler.noise_level(timestep)
        a_t = float(self.scheduler.alphas_cumprod[int(timestep)])
        return a_t ** 0.5, (1.0 - a_t) ** 0.5

    def renoise_table(self, timesteps):
        """fp32 [len(timesteps), 2]: the coefficient table of `K.masked_renoise`.  The scheduler-step kernels have already advanced the
        step counter when the blend reads it, and they wrap it to 0 after the last row: row 0 = (1, 0), the clean source after the
        last step; row r >= 1 = (sqrt(abar), sqrt(1 - abar)) of timesteps[r], the level the next step expects.  A one-step schedule
        falls on row 0."""
        rows = [(1.0, 0.0)] + [self._noise_level(t) for t in list(timesteps)[1:]]
        return torch.tensor(rows, dtype=torch.float32)

    def prepare_mask_latents(self, mask_image, batch_size, num_frames, height, width):
        """-> fp32 [batch_size, num_frames, 1, height / 8, width / 8] on the host; 1 regenerates, 0 keeps the source.  `mask_image`: one
        PIL image or [H, W] tensor for all frames, `num_frames` PIL images, [F, 1, H, W] or [B, F, 1, H, W] (values in [0, 1]; frames
        beyond `num_frames` are dropped).  Converted to grey, resized to height x width (PIL: Lanczos; tensors: nearest), binarised at
        >= 0.5, then taken to the latent resolution by torch.nn.functional.interpolate(mode="nearest").  A tensor already at
        (height / 8, width / 8) is taken as it is, unbinarised: soft masks are allowed."""
        import PIL.Image
        import torch.nn.functional as F
        h, w = height // self.vae_scale_factor, width // self.vae_scale_factor
        if isinstance(mask_image, PIL.Image.Image):
            mask_image = [mask_image]
        if isinstance(mask_image, (list, tuple)):
            planes = [_pil_plane(im, "mask_image", "L", height, width) for im in mask_image]
            t = torch.stack(planes)[None, :, None]                                          # [1, F or 1, 1, H, W]
        elif isinstance(mask_image, torch.Tensor):
            t = mask_image.detach().float().cpu()
            if t.dim() == 2:
                t = t[None, None, None]
            elif t.dim() == 4 and t.shape[1] == 1:
                t = t[None]
            elif not (t.dim() == 5 and t.shape[2] == 1):
                raise ValueError(f"`mask_image` must be [H, W], [F, 1, H, W] or [B, F, 1, H, W], got {tuple(mask_image.shape)}")
        else:
            raise ValueError(f"`mask_image` must be a PIL image, a list of `num_frames` PIL images or a tensor, got {type(mask_image)}")
        if t.shape[1] == 1:
            t = t.expand(-1, num_frames, -1, -1, -1)
        if t.shape[1] < num_frames:
            raise ValueError(f"`mask_image` holds {t.shape[1]} frames, `num_frames` is {num_frames}")
        t = t[:, :num_frames]
        if t.shape[0] == 1:
            t = t.expand(batch_size, -1, -1, -1, -1)
        if t.shape[0] != batch_size:
            raise ValueError(f"`mask_image` {tuple(t.shape)} does not match batch {batch_size}")
        flat = t.reshape(batch_size * num_frames, 1, *t.shape[-2:])
        if tuple(flat.shape[-2:]) != (h, w):
            if tuple(flat.shape[-2:]) != (height, width):
                flat = F.interpolate(flat, size=(height, width), mode="nearest")
            flat = F.interpolate((flat >= 0.5).to(torch.float32), size=(h, w), mode="nearest")
        return flat.reshape(batch_size, num_frames, 1, h, w).contiguous()

    # ------------------------------------------------------------------------------------------ encode_image
    def encode_image(self, image, device, num_images_per_prompt, output_hidden_states=None):
        """pipe:323-345, both branches: a non-tensor image goes through `self.feature_extractor` (resize, crop and normalisation stay
        on the host, as tokenisation does), the image encoder (clip_vision.CLIPVisionModelWithProjection on the HIP kernels), the
        per-prompt repeat.  Returns (image_embeds, zeros_like) -- or, with `output_hidden_states`, the penultimate hidden states of the
        image and of a zero image."""
        if self.image_encoder is None:
            raise ValueError("encoding an image needs an `image_encoder`: build the pipeline with one, or `load_ip_adapter` from a "
                             "folder that holds `image_encoder/`")
        dtype = next(self.image_encoder.parameters()).dtype
        if not isinstance(image, torch.Tensor):
            if self.feature_extractor is None:
                raise ValueError("an `ip_adapter_image` that is not a pixel_values tensor needs a `feature_extractor` (transformers' "
                                 "CLIPImageProcessor, or any object with its call interface)")
            image = self.feature_extractor(image, return_tensors="pt").pixel_values
        image = image.to(device=device, dtype=dtype)
        if output_hidden_states:
            image_enc_hidden_states = self.image_encoder(image, output_hidden_states=True).hidden_states[-2]
            image_enc_hidden_states = image_enc_hidden_states.repeat_interleave(num_images_per_prompt, dim=0)
            uncond_image_enc_hidden_states = self.image_encoder(torch.zeros_like(image), output_hidden_states=True).hidden_states[-2]
            uncond_image_enc_hidden_states = uncond_image_enc_hidden_states.repeat_interleave(num_images_per_prompt, dim=0)
            return image_enc_hidden_states, uncond_image_enc_hidden_states
        image_embeds = self.image_encoder(image).image_embeds
        image_embeds = image_embeds.repeat_interleave(num_images_per_prompt, dim=0)
        uncond_image_embeds = torch.zeros_like(image_embeds)
        return image_embeds, uncond_image_embeds

    # ------------------------------------------------------------------------------------------ encode_prompt
    def encode_prompt(self, prompt, device, num_images_per_prompt, do_classifier_free_guidance, negative_prompt=None,
                      prompt_embeds=None, negative_prompt_embeds=None, lora_scale=None, clip_skip=None):
        """pipe:348-527, line for line: tokenise (padding to `model_max_length`, truncation with the reference's warning), the text
        encoder (clip_text.CLIPTextModel on the HIP kernels), `clip_skip` (`hidden_states[-(clip_skip + 1)]` through
        `final_layer_norm`), the per-prompt repeat, and the negative prompt ("" when none is given) under classifier-free guidance.
        Returns (prompt_embeds, negative_prompt_embeds).  `lora_scale` is accepted and ignored (text-encoder LoRA keys are skipped and
        reported by `load_lora_weights`).  Textual inversion: `maybe_convert_prompt` on the prompt and on the negative prompt, as the
        reference does (pipe:409, 491); with nothing loaded it returns them unchanged.  `self.tokenizer` is used as given: any object
        with CLIPTokenizer's call interface and `model_max_length`.  A prompt beyond 77 tokens is truncated and `(text:1.3)` is literal
        text here: `enable_prompt_weighting` / `encode_weighted_prompt` is the path for long and weighted prompts."""
        if prompt is not None and isinstance(prompt, str):
            batch_size = 1
        elif prompt is not None and isinstance(prompt, list):
            batch_size = len(prompt)
        else:
            batch_size = prompt_embeds.shape[0]
        needs_encoder = prompt_embeds is None or (do_classifier_free_guidance and negative_prompt_embeds is None)
        if needs_encoder:
            self._require_text_encoder()

        if prompt_embeds is None:
            prompt = self.maybe_convert_prompt(prompt, self.tokenizer)                          # pipe:409 (textual inversion)
            text_inputs = self.tokenizer(prompt, padding="max_length", max_length=self.tokenizer.model_max_length, truncation=True,
                                         return_tensors="pt")
            text_input_ids = text_inputs.input_ids
            untruncated_ids = self.tokenizer(prompt, padding="longest", return_tensors="pt").input_ids
            if untruncated_ids.shape[-1] >= text_input_ids.shape[-1] and not torch.equal(text_input_ids, untruncated_ids):
                removed_text = self.tokenizer.batch_decode(untruncated_ids[:, self.tokenizer.model_max_length - 1: -1])
                logger.warning("The following part of your input was truncated because CLIP can only handle sequences up to"
                               f" {self.tokenizer.model_max_length} tokens: {removed_text}")
            prompt_embeds = self._embed_ids(text_input_ids, clip_skip)                          # pipe:438-453

        if self.text_encoder is not None:
            prompt_embeds_dtype = self.text_encoder.dtype
        elif self.unet is not None:
            prompt_embeds_dtype = self.unet.dtype
        else:
            prompt_embeds_dtype = prompt_embeds.dtype
        prompt_embeds = prompt_embeds.to(dtype=prompt_embeds_dtype, device=device)
        bs_embed, seq_len, _ = prompt_embeds.shape
        prompt_embeds = prompt_embeds.repeat(1, num_images_per_prompt, 1)
        prompt_embeds = prompt_embeds.view(bs_embed * num_images_per_prompt, seq_len, -1)

        if do_classifier_free_guidance and negative_prompt_embeds is None:
            if negative_prompt is None:
                uncond_tokens = [""] * batch_size
            elif prompt is not None and type(prompt) is not type(negative_prompt):
                raise TypeError(f"`negative_prompt` should be the same type to `prompt`, but got {type(negative_prompt)} !="
                                f" {type(prompt)}.")
            elif isinstance(negative_prompt, str):
                uncond_tokens = [negative_prompt]
            elif batch_size != len(negative_prompt):
                raise ValueError(f"`negative_prompt`: {negative_prompt} has batch size {len(negative_prompt)}, but `prompt`:"
                                 f" {prompt} has batch size {batch_size}. Please make sure that passed `negative_prompt` matches"
                                 " the batch size of `prompt`.")
            else:
                uncond_tokens = negative_prompt
            uncond_tokens = self.maybe_convert_prompt(uncond_tokens, self.tokenizer)            # pipe:491 (textual inversion)
            max_length = prompt_embeds.shape[1]
            uncond_input = self.tokenizer(uncond_tokens, padding="max_length", max_length=max_length, truncation=True,
                                          return_tensors="pt")
            negative_prompt_embeds = self._embed_ids(uncond_input.input_ids)                    # (no clip_skip here: pipe:508-512)

        if do_classifier_free_guidance:
            seq_len = negative_prompt_embeds.shape[1]
            negative_prompt_embeds = negative_prompt_embeds.to(dtype=prompt_embeds_dtype, device=device)
            negative_prompt_embeds = negative_prompt_embeds.repeat(1, num_images_per_prompt, 1)
            negative_prompt_embeds = negative_prompt_embeds.view(batch_size * num_images_per_prompt, seq_len, -1)
        return prompt_embeds, negative_prompt_embeds

    # ------------------------------------------------------------------------------------------ prompt travel
    def _encode_texts(self, texts, clip_skip=None):
        """[len(texts), L, D]: the text encoder's embeddings of a list of strings in ONE call, as `encode_prompt` makes them (padding to
        `model_max_length`, truncation, `clip_skip` through the final LayerNorm)"""
        self._require_text_encoder()
        texts = self.maybe_convert_prompt(texts, self.tokenizer)
        ids = self.tokenizer(texts, padding="max_length", max_length=self.tokenizer.model_max_length, truncation=True,
                             return_tensors="pt").input_ids
        return self._embed_ids(ids, clip_skip)

    def encode_prompt_travel(self, prompt, num_frames, device, num_videos_per_prompt, do_classifier_free_guidance, negative_prompt=None,
                             clip_skip=None, interpolation_callback=None):
        """Prompt travel (diffusers AnimateDiffFreeNoiseMixin `_encode_prompt_free_noise`): `prompt` and `negative_prompt` are each a
        str, a keyframe dict {frame: text} (keys ints, the first 0, the last < num_frames; the last prompt is held to the end of the
        clip) or a list of either with one entry per sample.  Returns (prompt_embeds, negative_prompt_embeds), each
        [B * num_videos_per_prompt, num_frames, L, D] -- one context per frame; the second is None without classifier-free guidance.
        Every keyframe text of the batch, negative ones included, goes through the text encoder in ONE call (K rows), and ONE
        `K.interp_rows` launch makes all frames: frame f between the keyframes s < e gets (1 - w) E_s + w E_e with
        w = float32(linspace(0, 1, e - s + 1)[f - s]); a keyframe's own frame is its embedding bit for bit.
        interpolation_callback(start_frame, end_frame, start_embeds [L, D], end_embeds [L, D]) -> [end - start + 1, L, D] replaces the
        linear rule for that segment (diffusers' `prompt_interpolation_callback`; as there, a later segment's first row overwrites the
        shared keyframe's)."""
        from . import prompt_travel as PT
        if isinstance(prompt, (list, tuple)):
            batch = len(prompt)
        elif isinstance(negative_prompt, (list, tuple)):
            batch = len(negative_prompt)
        else:
            batch = 1
        if batch < 1:
            raise ValueError("`prompt` is an empty list")
        if prompt is None:
            raise ValueError("`prompt` is required")
        groups = [PT.per_sample_keyframes(prompt, batch, num_frames, "prompt")]
        if do_classifier_free_guidance:
            neg = "" if negative_prompt is None else negative_prompt
            groups.insert(0, PT.per_sample_keyframes(neg, batch, num_frames, "negative_prompt"))
        # the source rows: [negative keyframes of sample 0, 1, ... ; positive keyframes of sample 0, 1, ...], each sample's sorted by frame
        texts, keyframes = [], []
        for g in groups:
            for d in g:
                keys = sorted(d)
                keyframes.append(keys)
                texts.extend(d[k] for k in keys)
        dtype = self.text_encoder.dtype if self.text_encoder is not None else f16
        # (while prompt weighting is enabled the source rows are the weighted embeddings, [K, n * M, D]: every keyframe text of the
        # batch padded to the chunk count of the longest)
        encode = (lambda t, s: self._encode_weighted_texts([t], s)) if self._prompt_weighting is not None else self._encode_texts
        src = encode(texts, clip_skip).to(device=device, dtype=dtype).contiguous()
        if src.dtype != f16:
            raise HipLibraryError(f"prompt travel interpolates fp16 embeddings (i2v_interp_rows_f16), the text encoder gives {src.dtype}")
        lo, hi, w, n_src = PT.batch_tables(keyframes, num_frames, repeats=num_videos_per_prompt)
        if interpolation_callback is not None:
            # a segment's rows as the callback gives them: appended to the source, gathered with w = 0
            extra, base, row = [], 0, 0
            for keys in keyframes:
                for i, (s, e) in enumerate(zip(keys[:-1], keys[1:])):
                    seg = interpolation_callback(s, e, src[base + i], src[base + i + 1])
                    if not isinstance(seg, torch.Tensor) or tuple(seg.shape) != (e - s + 1,) + tuple(src.shape[1:]):
                        raise ValueError(f"interpolation_callback({s}, {e}, ...) must return a tensor {(e - s + 1,) + tuple(src.shape[1:])}, "
                                         f"got {tuple(seg.shape) if isinstance(seg, torch.Tensor) else type(seg).__name__}")
                    extra.append(seg.to(device=device, dtype=f16))
                    first = n_src + sum(t.shape[0] for t in extra[:-1])
                    for rep in range(num_videos_per_prompt):
                        r0 = row + rep * num_frames
                        lo[r0 + s: r0 + e + 1] = hi[r0 + s: r0 + e + 1] = range(first, first + e - s + 1)
                        w[r0 + s: r0 + e + 1] = 0.0
                base += len(keys)
                row += num_videos_per_prompt * num_frames
            if extra:
                src = torch.cat([src] + extra).contiguous()
        out = K.interp_rows(src, lo, hi, w).view(len(groups), batch * num_videos_per_prompt, num_frames, *src.shape[1:])
        return (out[1], out[0]) if do_classifier_free_guidance else (out[0], None)

    def _per_frame_embeds(self, embeds, num_frames, name):
        """`embeds` as per-frame contexts [B, num_frames, L, D] fp16 on the UNet's device: a 4-D tensor as it is (its frame count
        checked), a 3-D one [B, L, D] repeated for every frame (the w = 0 gather of K.interp_rows)"""
        if embeds.dim() == 4:
            if embeds.shape[1] != num_frames:
                raise ValueError(f"`{name}` is [B, F, L, D] = {tuple(embeds.shape)} with F = {embeds.shape[1]} per-frame contexts, "
                                 f"`num_frames` is {num_frames}")
            return embeds.to(self.unet.device, f16).contiguous()
        src = embeds.to(self.unet.device, f16).contiguous()
        rows = torch.arange(src.shape[0]).repeat_interleave(num_frames)
        return K.interp_rows(src, rows, rows, torch.zeros(rows.numel())).view(src.shape[0], num_frames, *src.shape[1:])

    # ------------------------------------------------------------------------------------------ __call__
    @torch.no_grad()
    def __call__(self, prompt=None, condition_image=None, num_frames: Optional[int] = 16,
                 height: Optional[int] = None, width: Optional[int] = None, num_inference_steps: int = 50,
                 guidance_scale: float = 7.5, negative_prompt=None, num_videos_per_prompt: Optional[int] = 1,
                 eta: float = 0.0, generator=None, latents=None, prompt_embeds=None, negative_prompt_embeds=None,
                 ip_adapter_image=None, output_type: Optional[str] = None, return_dict: bool = True,
                 callback=None, callback_steps: Optional[int] = 1, cross_attention_kwargs=None, clip_skip=None,
                 frame_similarity_sample_ratio: float = 1, frame_similarity_blurred_strength: float = 0.6,
                 condition_image_latents=None, image_embeds=None, negative_image_embeds=None,
                 prior_mask_generator=None, prior_noise_generator=None, blur_sigma: Optional[float] = None,
                 use_graph: bool = True, precise_stream: Optional[bool] = None, control_image=None,
                 controlnet_conditioning_scale: float = 1.0, control_guidance_start: float = 0.0, control_guidance_end: float = 1.0,
                 guess_mode: bool = False, adapter_image=None, adapter_conditioning_scale: float = 1.0,
                 adapter_conditioning_factor: float = 1.0, video=None, video_latents=None, strength: Optional[float] = None,
                 mask_image=None):
        """pipe:537-711 (the arguments the reference's `__call__` takes; `use_graph`, the explicit prior generators and
        `precise_stream` are additions, and so are the ControlNet arguments, which carry the names of diffusers'
        StableDiffusionControlNetPipeline: `control_image` -- `num_frames` PIL images, a [F, 3, H, W] tensor in [0, 1] shared by the
        batch or a [B, F, 3, H, W] tensor in [0, 1] --, `controlnet_conditioning_scale`, and the window
        `control_guidance_start` .. `control_guidance_end` of the schedule, as fractions, in which the control acts -- with a
        `MultiControlNetModel` of N nets `control_image` is a list of N such entries, each with its net's `conditioning_channels`,
        and the scale and the two window arguments are each a number for all nets or a list of N --; and the
        T2I-Adapter arguments of diffusers' StableDiffusionAdapterPipeline: `adapter_image` -- as `control_image`, with the adapter's
        `in_channels` --, `adapter_conditioning_scale`, and `adapter_conditioning_factor`, the fraction of the steps, from the
        first, on which the adapter's features are added).
        Prompt travel (diffusers' AnimateDiffFreeNoiseMixin): `prompt` and `negative_prompt` are each a str, a keyframe dict
        {frame: text} -- int keys, the first 0, the last < num_frames; the frames between two keyframes get interpolated embeddings
        (`encode_prompt_travel`) -- or a list of either with one entry per sample; `prompt_embeds` / `negative_prompt_embeds` may be
        4-D [B, num_frames, L, D], one context per frame.
        Video-to-video (diffusers' AnimateDiffVideoToVideoPipeline): `video` -- `num_frames` PIL images, a [F, 3, H, W] tensor in [0, 1]
        shared by the batch or [B, F, 3, H, W]; frames beyond `num_frames` are dropped -- is encoded by `encode_video`, or
        `video_latents` [B, F, 4, h, w] (already scaled) is taken as given; the clip starts from the source noised to the level of
        the first of the last int(num_inference_steps * strength) timesteps (`strength` in (0, 1], None: 0.8) instead of from the
        first-frame prior, and without a condition image the source's first frame is the condition.  `mask_image` (the inpainting
        pipelines': 1 regenerates, 0 keeps the source; one PIL image or [H, W] tensor for all frames, `num_frames` PIL images,
        [F, 1, H, W] or [B, F, 1, H, W]) adds one `K.masked_renoise` launch to the captured step.
        precise_stream: True / False runs THIS call with / without the precise residual stream
        (fp16 hi + lo pairs between the UNet's modules, DESIGN 2.2: closer to the fp32 reference, +2.6 % step time); None keeps the
        process setting (`blocks.set_precise_stream`, I2V_STREAM_PRECISE)."""
        with contextlib.ExitStack() as restore:
            # the per-call switches: set now, the previous values back on the way out (last set, first restored), also when the call raises
            if precise_stream is not None:
                restore.enter_context(_set_for_call(blocks.set_precise_stream, precise_stream))
            if cross_attention_kwargs and cross_attention_kwargs.get("scale") is not None:
                # the LoRA scale of THIS call (diffusers: cross_attention_kwargs={"scale": s}), before `_sync_lora` below.  A changed
                # scale re-merges the weights and so re-captures the step once (_graph_key hashes the weights' versions)
                restore.enter_context(_set_for_call(self.unet.set_lora_scale, cross_attention_kwargs["scale"]))
                cross_attention_kwargs = {k: v for k, v in cross_attention_kwargs.items() if k != "scale"}
            prompt, negative_prompt, travels, video, video_latents, strength = self._check_call_args(
                prompt, negative_prompt, prompt_embeds, negative_prompt_embeds, ip_adapter_image, image_embeds, num_frames,
                num_inference_steps, eta, frame_similarity_sample_ratio,
                (control_image, num_frames, controlnet_conditioning_scale, control_guidance_start, control_guidance_end, guess_mode),
                (adapter_image, num_frames, adapter_conditioning_scale, adapter_conditioning_factor),
                video, video_latents, strength, mask_image)
            output_type, use_graph = self._resolve_call_defaults(output_type, callback, use_graph)
            if self._upscaler is not None and output_type == "latent":
                raise ValueError("output_type='latent' with the upscaler enabled: nothing is decoded, so there is nothing to upscale "
                                 "(disable_upscaler(), or ask for 'pt' / 'pil' / 'np')")
            # the hires fix's target size and step count (None while it is disabled): its refusals come before anything is encoded
            hires = self._hires_target(height, width, condition_image, condition_image_latents, video, video_latents,
                                       num_inference_steps)
            given_condition_latents = condition_image_latents
            do_cfg = guidance_scale > 1.0
            self.unet._sync_lora()      # before anything reads a weight, a pack or the weights' versions (_graph_key)
            prompt_embeds, negative_prompt_embeds, image_embeds, negative_image_embeds = self._encode_contexts(
                prompt, negative_prompt, travels, prompt_embeds, negative_prompt_embeds, ip_adapter_image, image_embeds,
                negative_image_embeds, num_frames, num_videos_per_prompt, do_cfg, clip_skip,
                cross_attention_kwargs.get("scale", None) if cross_attention_kwargs is not None else None)
            batch_size = prompt_embeds.shape[0]
            height, width, condition_image_latents, video_latents = self._resolve_size_and_sources(
                condition_image, condition_image_latents, video, video_latents, height, width, batch_size, generator)
            assert 0 < frame_similarity_sample_ratio <= 1, (
                f'"frame_similarity_sample_ratio" for img2vid must in (0, 1]. But receive {frame_similarity_sample_ratio}.')
            prompt_embeds, image_embeds, per_frame = self._stack_guidance_halves(
                prompt_embeds, negative_prompt_embeds, image_embeds, negative_image_embeds, num_frames, do_cfg)
            round_steps = self._round_steps(num_inference_steps)
            latents, cond, noise, source, timesteps = self._initial_latents(
                condition_image_latents, video_latents, batch_size, num_frames, height, width, round_steps[0],
                frame_similarity_sample_ratio if video_latents is None else strength, frame_similarity_blurred_strength, generator,
                latents, prior_mask_generator, prior_noise_generator, blur_sigma)
            st = self._assemble_state(
                latents, cond, timesteps, eta, prompt_embeds, image_embeds, per_frame, 2 if do_cfg else 1, num_frames, guidance_scale,
                batch_size, height, width, control_image,
                self._control_args(controlnet_conditioning_scale, control_guidance_start, control_guidance_end), adapter_image,
                (float(adapter_conditioning_scale), float(adapter_conditioning_factor)), mask_image, source, noise, generator)
            latents = self._run_rounds(st, timesteps, round_steps, noise, use_graph, callback, callback_steps, eta, generator,
                                       frame_similarity_sample_ratio)
            if hires is not None:
                first = frame_similarity_sample_ratio if video_latents is None else strength
                steps_run = sum(min(int(n * first), n) for n in round_steps)
                latents = self._hires_pass(
                    hires, latents, steps_run, condition_image if given_condition_latents is None else None, condition_image_latents,
                    batch_size, num_frames, frame_similarity_blurred_strength, generator, prior_mask_generator, prior_noise_generator,
                    blur_sigma, eta, prompt_embeds, image_embeds, per_frame, 2 if do_cfg else 1, guidance_scale, control_image,
                    st.get("cn_args"), adapter_image, st.get("t2i_args"), mask_image, use_graph, callback, callback_steps)
            return self._output(latents, output_type, return_dict)

    # the phases of a call, in the order `__call__` runs them
    def _check_call_args(self, prompt, negative_prompt, prompt_embeds, negative_prompt_embeds, ip_adapter_image, image_embeds,
                         num_frames, num_inference_steps, eta, ratio, control_args, adapter_args, video, video_latents, strength,
                         mask_image):
        """Phase 1, the arguments: every check that needs no encoding, on the host, before anything is launched or encoded.  Reads the
        call's arguments (control_args / adapter_args: the argument lists of `_check_control_args` / `_check_adapter_args`) and the
        pipeline's parts and settings (FreeNoise, FreeInit).  Returns (prompt, negative_prompt, travels, video, video_latents,
        strength): the prompts with one-key keyframe dicts turned into their text, whether the call has keyframed prompts, the source
        clip cut to `num_frames` frames and the strength with its default."""
        self._check_control_args(*control_args)
        self._check_adapter_args(*adapter_args)
        # frames beyond num_frames are dropped here
        video, video_latents, strength = self._check_video_args(video, video_latents, strength, mask_image, num_frames,
                                                                num_inference_steps, ratio, eta)
        # prompt travel: a keyframe dict with one key is its text
        from .prompt_travel import normalize_prompt
        prompt, travels = normalize_prompt(prompt, num_frames, "prompt")
        negative_prompt, neg_travels = normalize_prompt(negative_prompt, num_frames, "negative_prompt")
        for name, t in (("prompt_embeds", prompt_embeds), ("negative_prompt_embeds", negative_prompt_embeds)):
            if t is not None and t.dim() == 4 and t.shape[1] != num_frames:
                raise ValueError(f"`{name}` is [B, F, L, D] = {tuple(t.shape)} with F = {t.shape[1]} per-frame contexts, `num_frames` is "
                                 f"{num_frames}")
        # FreeNoise (enable_free_noise): the settings against this call's num_frames
        fnz = self._free_noise_settings()
        if fnz is not None:
            from .free_init import MAX_FRAMES, MAX_HW
            from .free_noise import check_num_frames
            check_num_frames(num_frames, fnz)
            if self._free_init is not None and num_frames > MAX_FRAMES:
                raise ValueError(f"FreeNoise with FreeInit: num_frames {num_frames} exceeds FreeInit's {MAX_FRAMES} x {MAX_HW} x {MAX_HW} "
                                 "limit (frames x latent height x width of i2v_freeinit_mix) -- disable_free_init() for longer clips")
        if ip_adapter_image is not None:
            if image_embeds is not None:
                raise ValueError("Cannot forward both `ip_adapter_image` and `image_embeds`. Please make sure to only forward one of "
                                 "the two.")
            if self.image_encoder is None:
                raise NotImplementedError(
                    "`ip_adapter_image` needs an image encoder and this pipeline has none: `load_ip_adapter(path, subfolder=...)` loads "
                    "`<path>/<subfolder>/image_encoder` (IP-Adapter's `models/image_encoder`), or build the pipeline with "
                    "`image_encoder=CLIPVisionModelWithProjection.from_pretrained(...)`, or pass `image_embeds` (and "
                    "`negative_image_embeds`) instead")
            if self.unet.encoder_hid_proj is None:
                # (the reference encodes the image and the UNet then ignores it silently, unet:1351)
                raise ValueError("`ip_adapter_image` was passed but the UNet has no IP-Adapter: call `load_ip_adapter` first")
        if prompt is not None and prompt_embeds is not None:                                    # pipe:222-226
            raise ValueError(f"Cannot forward both `prompt`: {prompt} and `prompt_embeds`: {prompt_embeds}. Please make sure to"
                             " only forward one of the two.")
        if prompt is None and prompt_embeds is None:
            raise ValueError("Provide either `prompt` or `prompt_embeds`. Cannot leave both `prompt` and "
                             "`prompt_embeds` undefined.")
        if prompt is not None:                                                                  # pipe:595-609
            if not isinstance(prompt, (str, list, dict)):
                raise ValueError(f"`prompt` has to be of type `str`, `dict` or `list` but is {type(prompt)}")
            if self.text_encoder is None or self.tokenizer is None:
                raise ValueError("a `prompt` needs both a `text_encoder` and a `tokenizer`: build the pipeline with them, or pass "
                                 "`prompt_embeds` and `negative_prompt_embeds`")
        return prompt, negative_prompt, prompt is not None and (travels or neg_travels), video, video_latents, strength

    def _encode_contexts(self, prompt, negative_prompt, travels, prompt_embeds, negative_prompt_embeds, ip_adapter_image, image_embeds,
                         negative_image_embeds, num_frames, num_videos_per_prompt, do_cfg, clip_skip, lora_scale):
        """Phase 2, the text and image contexts: a `prompt` through the text encoder (keyframed: `encode_prompt_travel`; while prompt
        weighting is enabled: `encode_weighted_prompt`; else `encode_prompt`) and an `ip_adapter_image` through the image encoder,
        once per sample; embeddings that were passed in are taken as given (a given `negative_prompt_embeds` is kept beside an encoded
        prompt), `image_embeds` with their rank checked against the loaded IP-Adapter.  Returns (prompt_embeds,
        negative_prompt_embeds, image_embeds, negative_image_embeds), the halves of the guidance still apart."""
        dev = self.unet.device
        encode_negative = do_cfg and negative_prompt_embeds is None
        if travels:
            # keyframed prompts: one context per frame, [B, F, L, D]
            pe, ne = self.encode_prompt_travel(prompt, num_frames, dev, num_videos_per_prompt, encode_negative, negative_prompt,
                                               clip_skip=clip_skip)
            prompt_embeds, negative_prompt_embeds = pe, ne if negative_prompt_embeds is None else negative_prompt_embeds
        elif prompt is not None and self._prompt_weighting is not None:
            # weighted and long prompts: contexts of n * 77 rows
            pe, ne = self.encode_weighted_prompt(prompt, dev, num_videos_per_prompt, encode_negative, negative_prompt,
                                                 clip_skip=clip_skip)
            prompt_embeds, negative_prompt_embeds = pe, ne if negative_prompt_embeds is None else negative_prompt_embeds
        elif prompt is not None:
            prompt_embeds, negative_prompt_embeds = self.encode_prompt(
                prompt, dev, num_videos_per_prompt, do_cfg, negative_prompt, prompt_embeds=None,
                negative_prompt_embeds=negative_prompt_embeds, lora_scale=lora_scale, clip_skip=clip_skip)
        if ip_adapter_image is not None:                                                        # pipe:616-622
            # once per sample, before the step is captured.  ImageProjection (plain IP-Adapter) takes the pooled embeds and a zero
            # negative; a Resampler (IP-Adapter Plus) the penultimate hidden states of the image and of a zero image
            output_hidden_state = not isinstance(self.unet.encoder_hid_proj, ImageProjection)
            image_embeds, negative_image_embeds = self.encode_image(ip_adapter_image, dev, num_videos_per_prompt, output_hidden_state)
        elif image_embeds is not None and self.unet.encoder_hid_proj is not None:
            plus = isinstance(self.unet.encoder_hid_proj, Resampler)
            for name, t in (("image_embeds", image_embeds), ("negative_image_embeds", negative_image_embeds)):
                if t is not None and t.dim() != (3 if plus else 2):
                    raise ValueError(
                        f"`{name}` has shape {tuple(t.shape)}: " +
                        (f"IP-Adapter Plus is loaded (Resampler), which takes the image encoder's penultimate hidden states "
                         f"[batch, tokens, {self.unet.encoder_hid_proj.embed_dims}]" if plus else
                         "the plain IP-Adapter is loaded (ImageProjection), which takes the pooled image embeds [batch, embed_dim]"))
        return prompt_embeds, negative_prompt_embeds, image_embeds, negative_image_embeds

    def _resolve_size_and_sources(self, condition_image, condition_image_latents, video, video_latents, height, width, batch_size,
                                  generator):
        """Phase 3, the size and the encoded inputs: `height` / `width` from the arguments, the UNet's sample size or the condition
        latents; a `condition_image` and then a `video` through the VAE (in that order: each may draw from `generator`; a clip shared
        by the batch is encoded for every sample, each with its own draw); with a source clip and no condition its first frame is the
        condition.  Refuses a UNet that is not on the GPU.  Returns (height, width, condition_image_latents, video_latents)."""
        if (condition_image is not None and condition_image_latents is None) or video is not None:  # pipe:624-627
            if height is None or width is None:
                height = height or self.unet.config.sample_size * self.vae_scale_factor         # pipe:568-569
                width = width or self.unet.config.sample_size * self.vae_scale_factor
            if height % 8 != 0 or width % 8 != 0:                                               # pipe:213-214
                raise ValueError(f"`height` and `width` have to be divisible by 8 but are {height} and {width}.")
        if condition_image is not None and condition_image_latents is None:
            condition_image_latents = self.encode_condition_image(condition_image, height, width, generator)
        if video is not None:
            frames = self._video_frames(video, height, width)
            if frames.shape[0] == 1 and batch_size > 1:
                frames = frames.expand(batch_size, -1, -1, -1, -1)
            video_latents = self._encode_frames(frames, generator)
        if video_latents is not None and condition_image_latents is None:
            condition_image_latents = video_latents[:, 0]                 # the source's first frame is the condition
        if condition_image_latents is None:
            raise ValueError("`condition_image` (or `condition_image_latents`) is required: the reference's prior "
                             "(pipe:647-656) needs the condition image and crashes without it")
        if self.unet.device.type != "cuda":
            raise HipLibraryError(f"unet is on {self.unet.device}: the HIP path has no CPU fallback")
        h_lat, w_lat = condition_image_latents.shape[-2:]
        height = height or h_lat * self.vae_scale_factor
        width = width or w_lat * self.vae_scale_factor
        if height % 8 != 0 or width % 8 != 0:                                                   # pipe:213-214
            raise ValueError(f"`height` and `width` have to be divisible by 8 but are {height} and {width}.")
        # (latent sizes that are not multiples of 8 take the UNet's forward_upsample_size path, unet:1304-1311)
        return height, width, condition_image_latents, video_latents

    def _stack_guidance_halves(self, prompt_embeds, negative_prompt_embeds, image_embeds, negative_image_embeds, num_frames, do_cfg):
        """between phases 3 and 4, the contexts as the step's batch reads them: per-frame contexts (prompt travel, or 4-D embeds passed
        in) made [B, F, L, D] on both sides of the guidance, then under classifier-free guidance [negative ; positive] along the
        batch, for the image embeds too (a missing negative is zeros).  Returns (prompt_embeds, image_embeds, per_frame)."""
        per_frame = prompt_embeds.dim() == 4 or (do_cfg and negative_prompt_embeds is not None and negative_prompt_embeds.dim() == 4)
        if per_frame:
            prompt_embeds = self._per_frame_embeds(prompt_embeds, num_frames, "prompt_embeds")
            if do_cfg and negative_prompt_embeds is not None:
                negative_prompt_embeds = self._per_frame_embeds(negative_prompt_embeds, num_frames, "negative_prompt_embeds")
        if do_cfg:
            if negative_prompt_embeds is None:
                raise ValueError("classifier-free guidance needs `negative_prompt_embeds`")
            if prompt_embeds.shape != negative_prompt_embeds.shape:
                raise ValueError("`prompt_embeds` and `negative_prompt_embeds` must have the same shape when passed "
                                 f"directly, but got: `prompt_embeds` {prompt_embeds.shape} != "
                                 f"`negative_prompt_embeds` {negative_prompt_embeds.shape}.")
            prompt_embeds = torch.cat([negative_prompt_embeds, prompt_embeds])                  # pipe:613-614
            if image_embeds is not None:
                if negative_image_embeds is None:
                    negative_image_embeds = torch.zeros_like(image_embeds)                      # pipe:343
                image_embeds = torch.cat([negative_image_embeds, image_embeds])                 # pipe:621-622
        return prompt_embeds, image_embeds, per_frame

    def _round_steps(self, num_inference_steps):
        """the step count of every sampling round: one round, or FreeInit's `num_iters` (enable_free_init), where with fast sampling
        round i has its own, shorter schedule"""
        fi = self._free_init
        rounds = fi["num_iters"] if fi is not None else 1
        if fi is not None and fi["use_fast_sampling"] and rounds > 1:
            from .free_init import round_inference_steps
            return [round_inference_steps(num_inference_steps, rounds, i) for i in range(rounds)]
        return [num_inference_steps] * rounds

    def _initial_latents(self, condition_image_latents, video_latents, batch_size, num_frames, height, width, num_steps, strength,
                         blurred_strength, generator, latents, prior_mask_generator, prior_noise_generator, blur_sigma, lowres=None):
        """Phase 4, the first round's schedule and the latents it starts from.  `strength`: the fraction of the `num_steps` schedule
        that runs (the similarity ratio without a source clip).  The draws, in this order: `prepare_latents` (`generator`), the blur
        sigma and the prior's mask (`prior_mask_generator`; neither with a source clip), the noise (`prior_noise_generator`;
        rescheduled by FreeNoise behind its first window).  Without a source clip the first-frame-similarity prior + add_noise
        (pipe:647-656) in ONE HIP kernel -- the reference overwrites the latents drawn above (its `latents = self.scheduler.
        add_noise(...)`, pipe:656), and so does this; its random draws take explicit generators (the reference uses the unseeded
        global RNG) --, with one the source noised to the first timestep's level.  `lowres` (the hires fix's second pass, with
        `video_latents` None): (clip, tables, keep) -- the source is `K.resize_renoise(clip, tables)`, materialised only when `keep`
        (a mask's blend reads it), and the latents are ONE fused launch of the same kernel with the noise and the first timestep's
        level, the bits of the upscale followed by `prepare_video_latents`.  Returns (latents, cond, noise, source, timesteps):
        fp32 on the UNet's device, `source` None without a clip."""
        dev = self.unet.device
        has_clip = video_latents is not None or lowres is not None
        self.scheduler.set_timesteps(num_steps)                                                 # pipe:630-631
        timesteps, _ = self.get_timesteps(num_steps, strength)
        cond_dev = condition_image_latents.detach().to(dev, torch.float32).contiguous()
        latents = self.prepare_latents(batch_size, self.unet.config.in_channels, num_frames, height, width,
                                       torch.float32, dev, generator, latents)                  # pipe:635-645
        if blur_sigma is None and not has_clip:                                                 # pipe:112
            blur_sigma = draw_blur_sigma(prior_mask_generator[0] if isinstance(prior_mask_generator, (list, tuple))
                                         else prior_mask_generator)
        shape = (batch_size, num_frames) + tuple(cond_dev.shape[1:])
        source = None
        if lowres is not None:
            clip, tables, keep = lowres
            if tuple(clip.shape[:3]) != shape[:3] or (tables[0].shape[0], tables[2].shape[0]) != shape[3:]:
                raise ValueError(f"the first pass's latents are {tuple(clip.shape)}, the second pass's are {shape}")
            source = K.resize_renoise(clip, tables) if keep else None
        elif has_clip:
            source = video_latents.detach().to(dev, torch.float32)
            if source.shape[0] == 1 and batch_size > 1:
                source = source.expand(batch_size, -1, -1, -1, -1)
            if tuple(source.shape) != shape:
                raise ValueError(f"the source clip's latents are {tuple(source.shape)}, the call's are {shape} "
                                 "(batch, num_frames, the condition latents' channels and size)")
            source = source.contiguous()
        else:
            mask_u = _draw(torch.rand, shape, prior_mask_generator, dev)                        # pipe:652
        fnz = self._free_noise_settings()
        if fnz is not None and num_frames > fnz.context_length:
            # FreeNoise: the frames behind the first window re-use its noise (repeated or shuffled: `free_noise.reschedule_noise`)
            from .free_noise import reschedule_noise
            noise = reschedule_noise(lambda shp, g: _draw(torch.randn, shp, g, dev), shape, fnz, prior_noise_generator)
        else:
            noise = _draw(torch.randn, shape, prior_noise_generator, dev)                       # pipe:655
        noise = noise.contiguous()
        if lowres is not None:
            latents = K.resize_renoise(lowres[0], lowres[1], noise.to(torch.float32), *self._noise_level(timesteps[0]))
        elif has_clip:
            latents = self.prepare_video_latents(source, noise, timesteps[0])
        else:
            latents = K.first_frame_prior(cond_dev, mask_u.contiguous(), noise, blur_sigma, blurred_strength,
                                          *self._prior_level(timesteps[0]))
        return latents, cond_dev, noise, source, timesteps

    def _schedule_tables(self, st, timesteps, eta):
        """the tables of a schedule, fp32 on the device of st["latents"], written into `st`: `t_table` and `coef`
        (`scheduler.step_coefficients`), and one row per executed step for each feature the state holds -- `cn_scale` (conditioning
        scale x diffusers' `controlnet_keep` window, from st["cn_args"]) with a ControlNet's `cn_cond`, `t2i_scale` (the adapter's scale
        on the first int(steps * factor) steps, from st["t2i_args"]) with a T2I-Adapter's `t2i_feats`, `v2v_coef` (`renoise_table`)
        with a mask.  Round 0 of a call and every round of FreeInit's fast sampling call it: the tables then change shape, and so
        does the graph key."""
        dev = st["latents"].device
        st["t_table"] = timesteps.to(torch.float32).to(dev)
        st["coef"] = self.scheduler.step_coefficients(timesteps, eta).to(dev)
        if st.get("cn_cond") is not None:
            from .controlnet import controlnet_keep_table
            if isinstance(st["cn_cond"], tuple):                  # several ControlNets: [N, steps], one row per net
                rows = [controlnet_keep_table(len(timesteps), *args) for args in st["cn_args"]]
            else:
                rows = controlnet_keep_table(len(timesteps), *st["cn_args"])
            st["cn_scale"] = torch.tensor(rows, dtype=torch.float32, device=dev)
        if st.get("t2i_feats") is not None:
            from .t2i_adapter import adapter_scale_table
            st["t2i_scale"] = torch.tensor(adapter_scale_table(len(timesteps), *st["t2i_args"]), dtype=torch.float32, device=dev)
        if st.get("v2v_mask") is not None:
            st["v2v_coef"] = self.renoise_table(timesteps).to(dev)

    def _assemble_state(self, latents, cond, timesteps, eta, prompt_embeds, image_embeds, per_frame, copies, num_frames, guidance_scale,
                        batch_size, height, width, control_image, cn_args, adapter_image, t2i_args, mask_image, source, noise, generator):
        """Phase 5, the state dict `st` of the captured step (SAMPLE_INPUTS and the launch scalars), everything on the device: the
        contexts (the IP-Adapter's image tokens projected here), once per sample the ControlNet's embedding of the control frames and
        the T2I-Adapter's feature maps, the mask at the latent resolution with the source and the noise its blend reads, the tables of
        the first round's schedule (`_schedule_tables`), DPM-Solver++'s history buffer and, last, LCM's noise table -- the one draw
        here, from `generator`, after the prior's.  cn_args / t2i_args are kept in `st` for later rounds' tables."""
        dev = latents.device
        st = dict(
            latents=latents, cond=cond, copies=copies, num_frames=num_frames, guidance=float(guidance_scale),
            step_idx=torch.zeros(1, dtype=torch.int32, device=dev),
            ctx_text=prompt_embeds.to(dev, f16).contiguous(),
            ctx_ip=self.unet._project_image_embeds(
                {"image_embeds": image_embeds.to(dev)} if image_embeds is not None else None))
        if per_frame:
            # the step's context is [copies * B * F, L, D] in the order (CFG half, sample, frame) -- the order of the token rows, so
            # every cross-attention runs with kv_group = 1; the IP-Adapter's image tokens, one set per sample, get one set per frame
            # (the fused kernel indexes them with the text's context index)
            st["ctx_text"] = st["ctx_text"].view(-1, *st["ctx_text"].shape[2:])
            st["ctx_ip"] = self.unet._expand_image_tokens(st["ctx_ip"], st["ctx_text"].shape[0])
        if self._multi_controlnet():
            # several ControlNets: as below per net, each with its own frames and channel count; `cn_cond` is the tuple of their tokens
            conds = []
            for net, image in zip(self.controlnet.nets, control_image):
                frames = self.prepare_control_image(image, batch_size, num_frames, height, width, net.config.conditioning_channels)
                tokens = net.embed_condition(frames.to(dev, f16))
                conds.append(K.duplicate_batch(tokens) if copies == 2 else tokens)
            st["cn_cond"], st["cn_args"] = tuple(conds), cn_args
        elif self.controlnet is not None:
            # once per sample: the embedding of the B * F control frames (duplicated for the second CFG half); the scale table comes
            # with the schedule's, and the ControlNet's context projection and time table are made where the UNet's are (_project_once)
            frames = self.prepare_control_image(control_image, batch_size, num_frames, height, width).to(dev, f16)
            tokens = self.controlnet.embed_condition(frames)
            st["cn_cond"], st["cn_args"] = K.duplicate_batch(tokens) if copies == 2 else tokens, cn_args
        if self.t2i_adapter is not None:
            # once per sample: the adapter's four feature maps of the B * F control frames (ONE copy: the step's add wraps around for
            # the second CFG half)
            frames = self.prepare_adapter_image(adapter_image, batch_size, num_frames, height, width).to(dev, f16)
            st["t2i_feats"], st["t2i_args"] = self.t2i_adapter.embed(frames), t2i_args
        if mask_image is not None:
            # the inpainting update: after every scheduler step the kept region goes back to the source at the NEXT step's noise level
            # (the same initial noise), after the last step to the clean source -- one launch inside the captured step (_step)
            st["v2v_mask"] = self.prepare_mask_latents(mask_image, batch_size, num_frames, height, width).to(dev).contiguous()
            st["v2v_source"], st["v2v_noise"] = source, noise
        self._schedule_tables(st, timesteps, eta)
        kind = self._scheduler_kind()
        if kind == "dpmsolver++":
            # the previous step's data prediction: the first step of a sample is first order and does not read it
            st["x0_prev"] = torch.empty_like(latents)
        if kind in ("lcm", "euler_ancestral"):
            # every step's fresh noise (diffusers draws it inside `step`, from `generator`, after prepare_latents' draw): one table per
            # sample, drawn after the prior's draws, read on the device by the step counter -- the steps stay captured
            st["noise"] = self.scheduler.step_noise(timesteps, tuple(latents.shape), generator, dev)
        return st

    def _run_rounds(self, st, timesteps, round_steps, init_noise, use_graph, callback, callback_steps, eta, generator, ratio):
        """Phase 6, the sampling rounds: one pass over `timesteps`, and with FreeInit one more per further entry of `round_steps`, each
        from `_free_init_round`'s re-initialised latents; after every round frame 0 is the condition again.  K / V^T of the context
        for all 16 cross-attention layers is projected once per sample where it is consumed (`_run_steps`: a graph-cache hit projects
        straight into the graph's static buffers).  DPM-Solver++ has no stochastic form here (the reference passes `eta` only to a
        scheduler whose step takes it, pipe:184-199), and LCM's step takes no eta either, its noise is in the table: with both `eta`
        is ignored and the steps stay captured.  Returns the final latents."""
        fixed = self._scheduler_kind() in ("dpmsolver++", "lcm", "euler", "euler_ancestral")
        for rnd in range(len(round_steps)):
            if rnd > 0:
                timesteps = self._free_init_round(st, rnd, round_steps, init_noise, generator, ratio, eta)
            self._sample_round(st, timesteps, use_graph, callback, callback_steps, eta, fixed, generator)
            latents = st["latents"]
            latents[:, 0] = st["cond"]                                                          # pipe:699-700
        return latents

    def _output(self, latents, output_type, return_dict):
        """Phase 7, the output: the latents as they are ("latent"), or decoded by the VAE -- and upscaled while `enable_upscaler` is
        on -- to a tensor ("pt") or through `tensor2vid`"""
        if output_type == "latent":                                                             # pipe:702-703
            video = latents
        else:
            video_tensor = self.decode_latents(latents)                                         # pipe:706
            if self._upscaler is not None:
                video_tensor = self.upscale_frames(video_tensor)
            video = video_tensor if output_type == "pt" else tensor2vid(video_tensor, self.image_processor,
                                                                        output_type=output_type)  # pipe:708-711
        if not return_dict:
            return (video,)
        return I2VAdapterPipelineOutput(frames=video)

    def _hires_target(self, height, width, condition_image, condition_image_latents, video, video_latents, num_inference_steps):
        """the hires fix of this call, checked on the host before anything is encoded: None while it is disabled, else (height, width,
        steps) of the second pass.  The first pass's size is found as phase 3 finds it (the arguments, the UNet's sample size or the
        latents that were passed in); what phase 3 itself refuses is left to it."""
        hf = self._hires_fix
        if hf is None:
            return None
        from .hires_fix import second_pass_steps, target_size
        if (condition_image is not None and condition_image_latents is None) or video is not None:
            height = height or self.unet.config.sample_size * self.vae_scale_factor
            width = width or self.unet.config.sample_size * self.vae_scale_factor
        else:
            lat = condition_image_latents if condition_image_latents is not None else video_latents
            if lat is None:
                return None
            height = height or lat.shape[-2] * self.vae_scale_factor
            width = width or lat.shape[-1] * self.vae_scale_factor
        steps = hf.num_inference_steps or num_inference_steps
        second_pass_steps(steps, hf.strength)
        return target_size(height, width, hf) + (steps,)

    def _hires_pass(self, hires, first, steps_run, condition_image, condition_image_latents, batch_size, num_frames, blurred_strength,
                    generator, prior_mask_generator, prior_noise_generator, blur_sigma, eta, prompt_embeds, image_embeds, per_frame,
                    copies, guidance_scale, control_image, cn_args, adapter_image, t2i_args, mask_image, use_graph, callback,
                    callback_steps):
        """The hires fix's second pass (enable_hires_fix), after the first pass's rounds: what a call with
        `video_latents=upscale_latents(first)`, `strength`, the target size and the condition at that size would do -- phases 4 to 6
        again, the same draws in the same order from the same generator objects, one plain round whatever FreeInit is set to.  In the
        order of the draws: a `condition_image` is encoded again at the target size (condition latents that were passed in, or that
        came from a source clip's first frame, are upscaled), then `_initial_latents`' draws, then `_assemble_state`'s -- where the
        control frames, the adapter's features and the mask are prepared again at the target size; with a mask the source the blend
        keeps is the upscaled first pass.  The contexts are the first pass's.  `callback` goes on counting after the `steps_run`
        steps of the first pass.  Returns the final latents."""
        from .hires_fix import device_tables
        height, width, steps = hires
        hf, dev, vsf = self._hires_fix, self.unet.device, self.vae_scale_factor
        if condition_image is not None:
            cond = self.encode_condition_image(condition_image, height, width, generator)
        else:
            cond = self.upscale_latents(condition_image_latents[:, None], height, width, hf.upscaler)[:, 0]
        clip = first.detach().to(dev, torch.float32).contiguous()
        tables = device_tables(clip.shape[-2], clip.shape[-1], height // vsf, width // vsf, hf.upscaler, dev)
        latents, cond, noise, source, timesteps = self._initial_latents(
            cond, None, batch_size, num_frames, height, width, steps, hf.strength, blurred_strength, generator, None,
            prior_mask_generator, prior_noise_generator, blur_sigma, lowres=(clip, tables, mask_image is not None))
        if self._multi_controlnet():                     # one entry per net, each resized like a single net's
            control_image = [self._frames_at(t, height, width) for t in control_image]
        control_image, adapter_image = (self._frames_at(t, height, width) for t in (control_image, adapter_image))
        st = self._assemble_state(latents, cond, timesteps, eta, prompt_embeds, image_embeds, per_frame, copies, num_frames,
                                  guidance_scale, batch_size, height, width, control_image, cn_args, adapter_image, t2i_args,
                                  mask_image, source, noise, generator)
        if callback is not None:
            user_callback = callback
            callback = lambda i, t, x: user_callback(steps_run + i, t, x)
        fixed = self._scheduler_kind() in ("dpmsolver++", "lcm", "euler", "euler_ancestral")
        self._sample_round(st, timesteps, use_graph, callback, callback_steps, eta, fixed, generator)
        latents = st["latents"]
        latents[:, 0] = st["cond"]
        return latents

    @staticmethod
    def _frames_at(frames, height, width):
        """control / adapter frames for the second pass: PIL images are resized where they are prepared; a tensor, which has to have
        the call's size already, is resized here on the host (bilinear, as preprocessing) -- None and lists pass through"""
        if not isinstance(frames, torch.Tensor) or tuple(frames.shape[-2:]) == (height, width):
            return frames
        import torch.nn.functional as F
        t = frames.detach().float().cpu()
        flat = F.interpolate(t.reshape(-1, *t.shape[-3:]), size=(height, width), mode="bilinear", align_corners=False)
        return flat.reshape(*t.shape[:-2], height, width)

    def _free_init_round(self, st, rnd, round_steps, init_noise, generator, ratio, eta):
        """FreeInit between round rnd - 1 and round rnd >= 1 (diffusers `_apply_free_init`), in the order of the draws: the fresh noise
        z_rand from the call's `generator` (after everything the previous round drew), this round's schedule and its tables under fast
        sampling (`_schedule_tables`), the
        mix -- st["latents"], the clip as the call would return it, re-noised with the round-0 noise to the level of this round's first
        timestep (the level the prior noises to, pipe:656, and the one the round's first step expects) and low-passed against z_rand
        --, then an LCM round's noise table.  The state goes through `_run_steps`' copy-in path like a new sample's: same graph key
        without fast sampling, so the rounds replay one captured step.  (DPM-Solver++: x0_prev needs no reset, a round's first step is
        first order.)  Returns the round's timesteps."""
        from .free_init import free_init_filter
        fi, prev, dev = self._free_init, st["latents"], st["latents"].device
        z_rand = _draw(torch.randn, tuple(prev.shape), generator, dev).to(torch.float32).contiguous()
        if fi["use_fast_sampling"]:
            self.scheduler.set_timesteps(round_steps[rnd])
        timesteps, _ = self.get_timesteps(round_steps[rnd], ratio)
        if fi["use_fast_sampling"]:
            self._schedule_tables(st, timesteps, eta)
        b, f, c, h, w = prev.shape
        lpf = free_init_filter((f, h, w), fi["method"], fi["order"], fi["spatial_stop_frequency"], fi["temporal_stop_frequency"], device=dev)
        st["latents"] = K.freeinit_mix(prev.contiguous(), init_noise.contiguous(), z_rand, lpf, *self._prior_level(timesteps[0]))
        if self._scheduler_kind() in ("lcm", "euler_ancestral"):
            st["noise"] = self.scheduler.step_noise(timesteps, tuple(prev.shape), generator, dev)
        st["step_idx"] = torch.zeros(1, dtype=torch.int32, device=dev)
        return timesteps

    def _sample_round(self, st, timesteps, use_graph, callback, callback_steps, eta, fixed, generator):
        """one sampling pass over `timesteps` (pipe:663-697): st["latents"] in, st["latents"] out"""
        dev = st["latents"].device
        if callback is None and (eta == 0.0 or fixed):
            st["latents"] = self._run_steps(st, len(timesteps), use_graph)
        else:
            # eager steps: a per-step host hook (pipe:693-697), and / or the stochastic DDIM update (eta > 0, pipe:550, 659-660:
            # sigma_t is out of the direction coefficient -- `step_coefficients(timesteps, eta)` -- and comes back as fresh noise,
            # one draw of the latents' shape per step from `generator` as diffusers' scheduler draws it)
            if eta != 0.0 and use_graph and not fixed:
                import warnings
                warnings.warn("eta > 0: the stochastic DDIM update draws fresh noise on the host every step, so the steps run as "
                              "eager launches instead of the captured hipGraph (about 2x the step time)", RuntimeWarning, stacklevel=3)
            sigmas = None if fixed else self.scheduler.step_sigmas(timesteps, eta)
            self._project_once(st)
            for i, t in enumerate(timesteps):                                                   # pipe:666-697
                self._step(st)
                if eta > 0 and not fixed:
                    z = _draw(torch.randn, tuple(st["latents"].shape), generator, dev).to(torch.float32).contiguous()
                    K.axpby(st["latents"], z, 1.0, sigmas[i])
                if callback is not None and i % callback_steps == 0:
                    callback(i, t, st["latents"])


SCHEDULERS = ("ddim", "dpmsolver++")
STOCHASTIC_SCHEDULERS = ("lcm",)       # samplers whose step draws noise (from a device table: still one captured step)
SIGMA_SCHEDULERS = ("euler_discrete", "euler_ancestral")    # samplers in sigma space: Euler, and Euler-ancestral (noise from a table too)


def load_scheduler(model_path, kind="ddim", karras_sigmas=False):
    """the evaluation driver's scheduler (`--scheduler`) from `<model_path>/scheduler/scheduler_config.json`: "ddim" as the
    reference builds it (pipe:755-757), "dpmsolver++" the same config as a DPMSolverMultistepScheduler (DPM-Solver++(2M),
    linspace spacing, steps_offset=1), "lcm" the same config as an LCMScheduler (the checkpoint's betas, diffusers' LCM defaults for the
    rest: for a UNet with an LCM-LoRA or AnimateLCM merged in), "euler_discrete" / "euler_ancestral" the same config as an
    EulerDiscreteScheduler (`karras_sigmas`: with Karras et al.'s noise levels) / EulerAncestralDiscreteScheduler, linspace spacing and
    steps_offset=1 as the DDIM line has."""
    if kind == "ddim":
        return DDIMScheduler.from_pretrained(model_path, subfolder="scheduler", clip_sample=False,
                                             timestep_spacing="linspace", steps_offset=1)          # pipe:755-757
    if kind == "dpmsolver++":
        return DPMSolverMultistepScheduler.from_pretrained(model_path, subfolder="scheduler", timestep_spacing="linspace",
                                                           steps_offset=1)
    if kind == "lcm":
        return LCMScheduler.from_pretrained(model_path, subfolder="scheduler", timestep_spacing="leading", steps_offset=0,
                                            set_alpha_to_one=True, clip_sample=False)
    if kind == "euler_discrete":
        return EulerDiscreteScheduler.from_pretrained(model_path, subfolder="scheduler", timestep_spacing="linspace", steps_offset=1,
                                                      use_karras_sigmas=bool(karras_sigmas))
    if kind == "euler_ancestral":
        return EulerAncestralDiscreteScheduler.from_pretrained(model_path, subfolder="scheduler", timestep_spacing="linspace",
                                                               steps_offset=1)
    raise ValueError(f"unknown scheduler {kind!r}: one of {', '.join(SCHEDULERS + STOCHASTIC_SCHEDULERS + SIGMA_SCHEDULERS)}")


def load_text_encoder(model_path):
    """(text_encoder, tokenizer) of an SD-1.5 folder (pipe:752-753): `<model_path>/text_encoder` as the HIP `CLIPTextModel`,
    `<model_path>/tokenizer` as transformers' `CLIPTokenizer` (there is no tokenizer of our own; nothing is downloaded)."""
    from .clip_text import CLIPTextModel
    try:
        from transformers import CLIPTokenizer
    except ImportError as e:
        raise ImportError("encoding prompts needs the `transformers` package for CLIPTokenizer (the tokenizer is not part of this "
                          "build): install it, or pass --embeds with precomputed embeddings") from e
    tokenizer = CLIPTokenizer.from_pretrained(os.path.join(model_path, "tokenizer"), local_files_only=True)
    return CLIPTextModel.from_pretrained(os.path.join(model_path, "text_encoder")), tokenizer


def build_parser():
    """the evaluation driver's command line (`main`)"""
    import argparse
    parser = argparse.ArgumentParser()
    parser.add_argument("--checkpoint_epoch", type=int, default=0)
    parser.add_argument("--eval_data_path", type=str, default="./data/WebVid-10M/I2VAdapter-eval.csv")
    parser.add_argument("--task_name", type=str)
    parser.add_argument("--embeds", type=str, default=None,
                        help="safetensors with prompt_embeds [N,77,768], negative_prompt_embeds [N or 1,77,768], "
                             "optional image_embeds [N,1024] (row i = CSV row i); without it the CSV's prompts are encoded by "
                             "<model_path>/text_encoder with <model_path>/tokenizer")
    parser.add_argument("--negative_prompt", type=str, default="",
                        help="the negative prompt of every row when the prompts are encoded here (no --embeds)")
    parser.add_argument("--prompt_travel_column", type=str, default=None, metavar="COL",
                        help="prompt travel: the CSV column that holds, per row, the keyframed prompts as JSON "
                             "{\"0\": \"...\", \"32\": \"...\"} (frame index -> prompt; the first key is 0, the last below num_frames); "
                             "the frames in between get interpolated embeddings.  An empty cell keeps the row's `name` prompt.  Not "
                             "with --embeds")
    parser.add_argument("--prompt_weighting", type=int, nargs="?", const=3, default=None, metavar="N",
                        help="weighted and long prompts (pipe.enable_prompt_weighting): `(text:1.3)` / `(text)` / `[text]` emphasis in the "
                             "prompts, the negative prompt and the keyframes of --prompt_travel_column, and prompts of up to N chunks of "
                             "75 tokens (3 when given without a value); off by default.  Not with --embeds")
    parser.add_argument("--textual_inversion", action="append", default=[], metavar="PATH[:TOKEN]",
                        help="a textual-inversion embedding (.safetensors / .bin / .pt; diffusers or A1111 format) added to the "
                             "tokenizer and the text encoder, with an optional token that replaces the file's; repeatable.  Not with "
                             "--embeds")
    parser.add_argument("--model_path", type=str, default="./SG161222_Realistic_Vision_V5.1_noVAE/")
    parser.add_argument("--motion_adapter_path", type=str, default="./animatediff-motion-adapter-v1-5-2")
    parser.add_argument("--ip_adapter_path", type=str, default="./IP-Adapter/")
    parser.add_argument("--ip_adapter", action="store_true",
                        help="load IP-Adapter and its CLIP image encoder from <ip_adapter_path>/models (pipe:783) and pass every row's "
                             "condition image as `ip_adapter_image` (pipe:796) unless --embeds holds image_embeds; off by default")
    parser.add_argument("--ip_adapter_weight_name", type=str, default="ip-adapter_sd15.bin",
                        help="the IP-Adapter file under <ip_adapter_path>/models: the plain adapter (4 image tokens) or an IP-Adapter "
                             "Plus file such as ip-adapter-plus_sd15.bin (16 image tokens through the Resampler)")
    parser.add_argument("--ip_adapter_scale", type=float, default=None,
                        help="weight of the image-prompt branch (pipe.set_ip_adapter_scale); default: the adapter's 1.0")
    parser.add_argument("--checkpoint_root", type=str, default="./checkpoint")
    parser.add_argument("--samples_root", type=str, default="./samples")
    parser.add_argument("--num_frames", type=int, default=16)
    parser.add_argument("--num_inference_steps", type=int, default=25)
    parser.add_argument("--height", type=int, default=None)
    parser.add_argument("--width", type=int, default=None)
    parser.add_argument("--seed", type=int, default=0)
    parser.add_argument("--scheduler", choices=SCHEDULERS + STOCHASTIC_SCHEDULERS, default="ddim",
                        help="ddim (the reference's), dpmsolver++ (DPM-Solver++(2M): 15-20 steps instead of 25-50) or lcm (latent-consistency "
                             "sampling for a UNet with an LCM-LoRA / AnimateLCM merged in (--lora): 4-8 steps, --guidance_scale 1-2)")
    parser.add_argument("--sampler", choices=SIGMA_SCHEDULERS, default=None,
                        help="a sampler in sigma space in place of --scheduler: euler_discrete (\"Euler\") or euler_ancestral (\"Euler a\": "
                             "fresh noise every step, from --seed).  (An option of its own: the choices of --scheduler are fixed.)")
    parser.add_argument("--karras_sigmas", action="store_true",
                        help="with --sampler euler_discrete: Karras et al.'s noise levels (use_karras_sigmas=True)")
    parser.add_argument("--guidance_scale", type=float, default=7.5, help="classifier-free guidance scale (pipe:794); <= 1 runs one copy")
    parser.add_argument("--freeu", type=float, nargs=4, default=None, metavar=("S1", "S2", "B1", "B2"),
                        help="enable FreeU with these scales (SD-1.5: 0.9 0.2 1.2 1.4); off by default, as in the reference driver")
    parser.add_argument("--lora", action="append", default=[], metavar="PATH[:WEIGHT]",
                        help="a LoRA file (.safetensors / .bin; diffusers, PEFT or kohya keys) merged into the UNet, with an optional "
                             "adapter weight; repeatable")
    parser.add_argument("--lora_scale", type=float, default=1.0, help="global LoRA scale (cross_attention_kwargs={'scale': S})")
    parser.add_argument("--vae_tiling", action="store_true",
                        help="tile the VAE decode / condition-image encode above 512 px a side (pipe.enable_vae_tiling(); off by "
                             "default, as in the reference driver)")
    parser.add_argument("--vae_tiny", type=str, default=None, metavar="PATH",
                        help="an AutoencoderTiny (TAESD) folder (config.json + diffusion_pytorch_model.safetensors) loaded in place of "
                             "<model_path>/vae: the cheap decode that goes with --scheduler lcm (no tiling: not with --vae_tiling)")
    parser.add_argument("--upscaler", type=str, default=None, metavar="PATH",
                        help="a Real-ESRGAN model -- compact (realesr-animevideov3 / realesr-general-x4v3) or RRDBNet (RealESRGAN_x4plus, "
                             "RealESRGAN_x4plus_anime_6B), picked by the file's keys: .pth, .pt or .safetensors -- run on the decoded "
                             "frames (pipe.enable_upscaler()): the GIFs are `upscale` x the size")
    parser.add_argument("--upscaler_act", type=str, default=None, choices=("prelu", "relu", "leakyrelu"),
                        help="with --upscaler: the activation of a file without PReLU weights (relu or leakyrelu)")
    parser.add_argument("--free_init", type=int, nargs="?", const=3, default=None, metavar="N",
                        help="FreeInit (pipe.enable_free_init): sample every clip N times (3 when given without a value), re-initialising "
                             "the noise's low frequencies from the previous round; off by default")
    parser.add_argument("--free_init_method", choices=("butterworth", "gaussian", "ideal"), default="butterworth",
                        help="FreeInit's low-pass filter")
    parser.add_argument("--free_noise", type=int, nargs="?", const=16, default=None, metavar="L",
                        help="FreeNoise (pipe.enable_free_noise): clips longer than the motion modules' 32 positions -- temporal attention "
                             "on sliding windows of L frames (16 when given without a value); off by default")
    parser.add_argument("--free_noise_stride", type=int, default=4, metavar="S", help="frames between two FreeNoise windows (4)")
    parser.add_argument("--free_noise_weighting", choices=("flat", "pyramid", "delayed_reverse_sawtooth"), default="pyramid",
                        help="FreeNoise's weights over the position in a window (diffusers' default: pyramid)")
    parser.add_argument("--free_noise_noise", choices=("shuffle_context", "repeat_context", "random"), default="shuffle_context",
                        help="FreeNoise's initial noise behind the first window (diffusers' default: shuffle_context)")
    parser.add_argument("--free_init_fast", action="store_true",
                        help="FreeInit's use_fast_sampling: earlier rounds take fewer steps (every round re-captures the step)")
    class OneOrList(argparse.Action):
        """a repeatable option: given once it is the value, as it always was; given again the values become a list"""

        def __call__(self, parser, namespace, value, option_string=None):
            seen = getattr(namespace, self.dest)
            setattr(namespace, self.dest, value if seen is None else (seen if isinstance(seen, list) else [seen]) + [value])

    parser.add_argument("--controlnet", type=str, default=None, metavar="PATH", action=OneOrList,
                        help="an SD-1.5 ControlNet folder (config.json + diffusion_pytorch_model.safetensors, e.g. "
                             "control_v11p_sd15_openpose): every clip follows the control frames of --control_column.  Repeatable "
                             "(Multi-ControlNet, up to 4): the n-th --controlnet reads the n-th --control_column")
    parser.add_argument("--control_column", type=str, default=None, metavar="NAME", action=OneOrList,
                        help="the CSV column that holds, per row, a directory of at least num_frames control images (taken in sorted "
                             "order) or an animated GIF, relative to the CSV; one per --controlnet")
    parser.add_argument("--controlnet_scale", type=float, default=1.0, metavar="S", nargs="+",
                        help="controlnet_conditioning_scale (1.0): one value for all nets or one per --controlnet")
    parser.add_argument("--control_guidance_start", type=float, default=0.0, metavar="A", nargs="+",
                        help="fraction of the schedule at which the control starts to act (0.0): one value or one per --controlnet")
    parser.add_argument("--control_guidance_end", type=float, default=1.0, metavar="B", nargs="+",
                        help="fraction of the schedule at which the control stops acting (1.0): one value or one per --controlnet")
    parser.add_argument("--t2i_adapter", type=str, default=None, metavar="PATH",
                        help="an SD-1.5 T2I-Adapter folder (config.json + diffusion_pytorch_model.safetensors, e.g. "
                             "t2iadapter_depth_sd15v2): every clip follows the control frames of --adapter_column, at no per-step "
                             "network cost")
    parser.add_argument("--adapter_column", type=str, default=None, metavar="COL",
                        help="the CSV column that holds, per row, a directory of at least num_frames control images (taken in sorted "
                             "order) or an animated GIF, relative to the CSV")
    parser.add_argument("--adapter_scale", type=float, default=1.0, metavar="S", help="adapter_conditioning_scale (1.0)")
    parser.add_argument("--adapter_factor", type=float, default=1.0, metavar="F",
                        help="adapter_conditioning_factor: the fraction of the steps, from the first, on which the adapter acts (1.0)")
    parser.add_argument("--video_column", type=str, default=None, metavar="COL",
                        help="video-to-video: the CSV column that holds, per row, the source clip -- a directory of at least num_frames "
                             "frames (taken in sorted order) or an animated GIF, relative to the CSV; the clip starts from the noised "
                             "source instead of from the first-frame prior")
    parser.add_argument("--strength", type=float, default=None, metavar="S",
                        help="with --video_column: the fraction of the schedule the source is noised to, in (0, 1] (0.8); the last "
                             "int(num_inference_steps * S) steps run")
    parser.add_argument("--mask_column", type=str, default=None, metavar="COL",
                        help="with --video_column: the CSV column that holds, per row, the mask -- one image for all frames, or a "
                             "directory / animated GIF of num_frames masks; white is regenerated, black keeps the source")
    parser.add_argument("--hires_scale", type=float, default=None, metavar="S",
                        help="hires fix (pipe.enable_hires_fix): after the pass at --height x --width, upscale the latents by S (>= 1; "
                             "each side rounded to a multiple of 8), re-noise them and refine at that size; use --vae_tiling above 512 px")
    parser.add_argument("--hires_size", type=int, nargs=2, default=None, metavar=("H", "W"),
                        help="hires fix with the target size given in pixels (multiples of 8, not below the first pass); instead of "
                             "--hires_scale")
    parser.add_argument("--hires_strength", type=float, default=0.6, metavar="S",
                        help="hires fix: the fraction of the schedule the upscaled latents are noised to, in (0, 1] (0.6)")
    parser.add_argument("--hires_steps", type=int, default=None, metavar="N",
                        help="hires fix: the schedule of the second pass, of which the last int(N * strength) steps run "
                             "(default: --num_inference_steps)")
    parser.add_argument("--hires_upscaler", type=str, default="bicubic-antialiased",
                        help="hires fix: the latent upscaler -- nearest, nearest-exact, bilinear, bicubic, bilinear-antialiased or "
                             "bicubic-antialiased (pixel-space upscalers and ESRGAN-class networks are not implemented)")
    return parser


def load_mask_frames(path, num_frames):
    """the mask of a driver row: one grey PIL image for all frames (a single image file), or the first `num_frames` masks of a
    directory of images / an animated GIF (`load_control_frames`)"""
    import PIL.Image
    if os.path.isfile(path):
        with PIL.Image.open(path) as im:
            if getattr(im, "n_frames", 1) == 1:
                return im.convert("L")
    return load_control_frames(path, num_frames)


def load_control_frames(path, num_frames):
    """the first `num_frames` control frames of a directory of images (sorted by name) or of an animated GIF, as RGB PIL images"""
    import PIL.Image
    import PIL.ImageSequence
    if os.path.isdir(path):
        names = sorted(f for f in os.listdir(path) if f.lower().endswith((".png", ".jpg", ".jpeg", ".bmp", ".webp")))
        frames = [PIL.Image.open(os.path.join(path, f)).convert("RGB") for f in names[:num_frames]]
    elif os.path.isfile(path):
        with PIL.Image.open(path) as im:
            frames = [fr.convert("RGB") for i, fr in enumerate(PIL.ImageSequence.Iterator(im)) if i < num_frames]
    else:
        raise FileNotFoundError(f"control frames: {path} is neither a directory nor a file")
    if len(frames) < num_frames:
        raise ValueError(f"control frames: {path} holds {len(frames)} frames, num_frames is {num_frames}")
    return frames


def main(argv=None):
    """The reference's evaluation driver (pipe:721-809, the README command
    `python src/pipelines/pipeline_i2v_adapter.py --task_name ... --checkpoint_epoch ...`): load MotionAdapter /
    I2VAdapterModule / SD-1.5 UNet + VAE / IP-Adapter from the reference's directory layout, read the CSV of
    (image_path, name) pairs, sample 16 frames per pair and write one GIF per prompt.

    The CSV's prompts are encoded by the HIP CLIP text encoder (`<model_path>/text_encoder`, clip_text.py) with transformers'
    `CLIPTokenizer` (`<model_path>/tokenizer`), as the reference does (pipe:752-753).  With --embeds the per-row `prompt_embeds`,
    `negative_prompt_embeds` (and `image_embeds`) come from a safetensors file instead and neither is loaded.  With --ip_adapter the
    IP-Adapter and its CLIP image encoder (`<ip_adapter_path>/models/image_encoder`, clip_vision.py) are loaded and the condition
    image is the image prompt, as in the reference (pipe:783, 796); everything else follows the reference driver."""
    import logging
    import os

    import pandas as pd
    import PIL.Image
    from safetensors.torch import load_file

    from .blocks import MotionAdapter
    from .i2v_adapter import I2VAdapterModule
    from .image_processor import export_to_gif
    from .unet_motion_cross_frame_attn import UNet2DConditionModel
    from .vae import AutoencoderKL

    logger = logging.getLogger("i2v_adapter_pipeline")
    logging.basicConfig(level=logging.INFO)
    args = build_parser().parse_args(argv)
    if args.task_name is None:
        logger.error("Checkpoint `task_name` must be specified.")
        return -1

    if (args.controlnet is None) != (args.control_column is None):
        logger.error("--controlnet and --control_column come together.")
        return -1
    as_list = lambda v: [] if v is None else v if isinstance(v, list) else [v]
    args.controlnet, args.control_column = as_list(args.controlnet) or None, as_list(args.control_column) or None
    n_nets = len(args.controlnet or [])
    if n_nets != len(args.control_column or []):
        logger.error(f"{n_nets} --controlnet and {len(args.control_column)} --control_column: each ControlNet reads its own column.")
        return -1
    for flag in ("controlnet_scale", "control_guidance_start", "control_guidance_end"):
        values = as_list(getattr(args, flag))
        if len(values) not in (1, max(n_nets, 1)):
            logger.error(f"--{flag} takes one value or one per --controlnet ({n_nets}), got {len(values)}.")
            return -1
        if n_nets <= 1 or len(values) == 1:                # one net, or one value for all nets: the plain number
            setattr(args, flag, values[0])
    if (args.t2i_adapter is None) != (args.adapter_column is None):
        logger.error("--t2i_adapter and --adapter_column come together.")
        return -1
    if args.prompt_travel_column is not None and args.embeds is not None:
        logger.error("--prompt_travel_column needs the text encoder: it is not combined with --embeds.")
        return -1
    if args.embeds is not None and (args.prompt_weighting is not None or args.textual_inversion):
        flag = "--prompt_weighting" if args.prompt_weighting is not None else "--textual_inversion"
        logger.error(f"{flag} needs the text encoder: it is not combined with --embeds.")
        return -1
    if args.prompt_weighting is not None and args.prompt_weighting < 1:
        logger.error(f"--prompt_weighting {args.prompt_weighting}: the number of chunks is at least 1.")
        return -1
    if args.karras_sigmas and args.sampler != "euler_discrete":
        logger.error("--karras_sigmas goes with --sampler euler_discrete.")
        return -1
    if args.video_column is None and (args.strength is not None or args.mask_column is not None):
        logger.error("--strength and --mask_column need a source clip: --video_column.")
        return -1
    hires = None
    if args.hires_scale is not None or args.hires_size is not None:
        from .hires_fix import check_hires_fix_args
        try:
            hires = check_hires_fix_args(args.hires_scale, args.hires_size, args.hires_strength, args.hires_steps, args.hires_upscaler)
        except ValueError as e:
            logger.error(f"--hires_scale / --hires_size: {e}")
            return -1
    i2v_adapter = None
    motion_adapter = MotionAdapter.from_pretrained(args.motion_adapter_path)                     # pipe:734
    checkpoint_path = os.path.join(args.checkpoint_root, args.task_name, f"epoch_{args.checkpoint_epoch}")
    i2v_adapter_path = os.path.join(checkpoint_path, "i2v_adapter")
    if not os.path.exists(i2v_adapter_path):
        logger.warning(f"Fatal! Checkpoint path {i2v_adapter_path} for I2VAdapterModule doesnot exist!")
    else:
        i2v_adapter = I2VAdapterModule.from_pretrained(i2v_adapter_path)                         # pipe:741
        logger.info(f"Successfully loaded I2VAdapterModule from {i2v_adapter_path}.")
    motion_adapter_path = os.path.join(checkpoint_path, "motion_modules")
    if os.path.exists(motion_adapter_path):
        motion_adapter = MotionAdapter.from_pretrained(motion_adapter_path)                      # pipe:745
        logger.info(f"Successfully loaded MotionModule from {motion_adapter_path}.")

    device = torch.device("cuda")                                # there is no CPU path (the reference falls back to it)
    unet2d = UNet2DConditionModel.from_pretrained(os.path.join(args.model_path, "unet"))         # pipe:751
    if args.vae_tiny is not None:
        from .autoencoder_tiny import AutoencoderTiny
        vae = AutoencoderTiny.from_pretrained(args.vae_tiny)
        logger.info(f"Successfully loaded AutoencoderTiny from {args.vae_tiny}.")
    else:
        vae = AutoencoderKL.from_pretrained(os.path.join(args.model_path, "vae"))                # pipe:754
    scheduler = load_scheduler(args.model_path, args.sampler or args.scheduler, karras_sigmas=args.karras_sigmas)   # pipe:755-757

    eval_data_dir = os.path.dirname(args.eval_data_path)                                         # pipe:759-768
    eval_data_df = pd.read_csv(args.eval_data_path)
    condition_images = [PIL.Image.open(os.path.join(eval_data_dir, p)) for p in eval_data_df["image_path"]]
    eval_prompts = eval_data_df["name"].tolist()
    n = len(eval_prompts)
    travel_prompts = [None] * n
    if args.prompt_travel_column is not None:
        # checked for every row before any model is loaded
        from .prompt_travel import check_keyframes, parse_travel_cell
        for i, cell in enumerate(eval_data_df[args.prompt_travel_column]):
            if isinstance(cell, str) and cell.strip():
                travel_prompts[i] = parse_travel_cell(cell)
                check_keyframes(travel_prompts[i], args.num_frames, f"{args.prompt_travel_column}[{i}]")
    text_encoder = tokenizer = None
    if args.embeds is not None:
        emb = load_file(args.embeds)
        if emb["prompt_embeds"].shape[0] != n:
            raise ValueError(f"{args.embeds} holds {emb['prompt_embeds'].shape[0]} prompt embeddings for {n} CSV rows")
    else:
        emb = {}
        text_encoder, tokenizer = load_text_encoder(args.model_path)                             # pipe:752-753

    controlnet = control_paths = None
    if args.controlnet is not None:
        from .controlnet import ControlNetModel, MultiControlNetModel
        nets = [ControlNetModel.from_pretrained(path) for path in args.controlnet]
        columns = [[os.path.join(eval_data_dir, str(p)) for p in eval_data_df[col]] for col in args.control_column]
        if len(nets) == 1:
            controlnet, control_paths = nets[0], columns[0]
        else:                                              # per row: one path per net
            controlnet, control_paths = MultiControlNetModel(nets), list(zip(*columns))
        logger.info(f"Successfully loaded ControlNetModel from {', '.join(args.controlnet)}.")
    t2i_adapter = adapter_paths = None
    if args.t2i_adapter is not None:
        from .t2i_adapter import T2IAdapter
        t2i_adapter = T2IAdapter.from_pretrained(args.t2i_adapter)
        adapter_paths = [os.path.join(eval_data_dir, str(p)) for p in eval_data_df[args.adapter_column]]
        logger.info(f"Successfully loaded T2IAdapter from {args.t2i_adapter}.")
    video_paths = mask_paths = None
    if args.video_column is not None:
        video_paths = [os.path.join(eval_data_dir, str(p)) for p in eval_data_df[args.video_column]]
        if args.mask_column is not None:
            mask_paths = [os.path.join(eval_data_dir, str(p)) for p in eval_data_df[args.mask_column]]
    pipe = I2VAdapterPipeline(vae, text_encoder, tokenizer, unet2d.to(device).half(), motion_adapter, i2v_adapter, scheduler,
                              controlnet=controlnet, t2i_adapter=t2i_adapter)
    if "image_embeds" in emb or args.ip_adapter:                                                 # pipe:783
        pipe.load_ip_adapter(args.ip_adapter_path, subfolder="models", weight_name=args.ip_adapter_weight_name)
        if args.ip_adapter_scale is not None:
            pipe.set_ip_adapter_scale(args.ip_adapter_scale)
    pipe.to(device, torch.float16)
    pipe.enable_vae_slicing()                                                                    # pipe:787
    for spec in args.textual_inversion:
        path, _, token = spec.rpartition(":") if ":" in spec and not os.path.exists(spec) else (spec, "", "")
        pipe.load_textual_inversion(path, token=token or None)
        logger.info(f"Successfully loaded the textual inversion {path}.")
    if args.prompt_weighting is not None:
        pipe.enable_prompt_weighting(max_embeddings_multiples=args.prompt_weighting)
    if args.freeu is not None:
        pipe.enable_freeu(*args.freeu)
    if args.vae_tiling:
        pipe.enable_vae_tiling()
    if args.upscaler is not None:
        pipe.enable_upscaler(args.upscaler, act_type=args.upscaler_act)
        logger.info(f"Successfully loaded the upscaler from {args.upscaler}.")
    if args.free_noise is not None:
        pipe.enable_free_noise(context_length=args.free_noise, context_stride=args.free_noise_stride,
                               weighting_scheme=args.free_noise_weighting, noise_type=args.free_noise_noise)
    if args.free_init is not None:
        pipe.enable_free_init(num_iters=args.free_init, use_fast_sampling=args.free_init_fast, method=args.free_init_method)
    if hires is not None:
        pipe.enable_hires_fix(scale=hires.scale, size=hires.size, strength=hires.strength,
                              num_inference_steps=hires.num_inference_steps, upscaler=hires.upscaler)
    if args.lora:
        names, weights = [], []
        for i, spec in enumerate(args.lora):
            path, _, w = spec.rpartition(":") if ":" in spec and not os.path.exists(spec) else (spec, "", "")
            rep = pipe.load_lora_weights(path, adapter_name=f"lora_{i}")
            names.append(rep["adapter_name"])
            weights.append(float(w) if w else 1.0)
            logger.info(f"LoRA {path}: {rep['modules']} UNet modules, {rep['text_encoder_keys']} text-encoder keys skipped")
        pipe.set_adapters(names, weights)
        pipe.unet.set_lora_scale(args.lora_scale)

    sample_save_dir = os.path.join(args.samples_root, args.task_name, f"epoch_{args.checkpoint_epoch}")
    os.makedirs(sample_save_dir, exist_ok=True)
    neg = emb.get("negative_prompt_embeds")
    for ind in range(n):                                         # one sample per call: every sample replays the graph
        g = lambda k: torch.Generator().manual_seed(args.seed * 1000 + 10 * ind + k)
        if args.embeds is not None:
            text = dict(prompt_embeds=emb["prompt_embeds"][ind: ind + 1],
                        negative_prompt_embeds=neg[ind: ind + 1] if neg.shape[0] == n else neg[:1])
        else:
            text = dict(prompt=travel_prompts[ind] if travel_prompts[ind] is not None else str(eval_prompts[ind]),
                        negative_prompt=args.negative_prompt)
        if "image_embeds" in emb:
            image = dict(image_embeds=emb["image_embeds"][ind: ind + 1])
        else:
            image = dict(ip_adapter_image=condition_images[ind]) if args.ip_adapter else {}      # pipe:796
        control = {}
        if controlnet is not None:
            paths = control_paths[ind]
            control = dict(control_image=load_control_frames(paths, args.num_frames) if isinstance(paths, str) else
                           [load_control_frames(p, args.num_frames) for p in paths],
                           controlnet_conditioning_scale=args.controlnet_scale, control_guidance_start=args.control_guidance_start,
                           control_guidance_end=args.control_guidance_end)
        if t2i_adapter is not None:
            control.update(adapter_image=load_control_frames(adapter_paths[ind], args.num_frames),
                           adapter_conditioning_scale=args.adapter_scale, adapter_conditioning_factor=args.adapter_factor)
        ratio = 0.9
        if video_paths is not None:
            # video-to-video: `strength` decides where the schedule starts, not the similarity ratio
            ratio = 1
            control.update(video=load_control_frames(video_paths[ind], args.num_frames), strength=args.strength)
            if mask_paths is not None:
                control.update(mask_image=load_mask_frames(mask_paths[ind], args.num_frames))
        out = pipe(**text, **image, **control,
                   condition_image=condition_images[ind], num_frames=args.num_frames, guidance_scale=args.guidance_scale,
                   num_inference_steps=args.num_inference_steps, frame_similarity_sample_ratio=ratio,
                   height=args.height, width=args.width, output_type="pil", generator=g(0),
                   prior_mask_generator=g(1), prior_noise_generator=g(2))                        # pipe:790-799
        export_to_gif(out.frames[0], os.path.join(sample_save_dir, f"{eval_prompts[ind]}.gif"))  # pipe:806-807
    logger.info(f"Finish sampling {n} instances, the results saved to {sample_save_dir}.")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
