"""The evaluation driver with `--ip_adapter --ip_adapter_weight_name ip-adapter-plus_sd15.bin` end to end on reduced models: the Plus
file is read from `<ip_adapter_path>/models`, every row's condition image goes through the image encoder's hidden states and the
Resampler, `--ip_adapter_scale` reaches every image branch, one GIF per prompt."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def test_eval_driver_with_a_plus_adapter(dev, tmp_path, monkeypatch):
    pytest.importorskip("transformers")
    import PIL.Image
    from safetensors.torch import save_file
    import i2v_adapter_unofficial_amd as p
    from i2v_adapter_unofficial_amd.checkpoint import init_random_weights_
    from i2v_adapter_unofficial_amd.pipeline_i2v_adapter import I2VAdapterPipeline, main
    from tests.clip_vision_reference import seeded_state
    from tests.ip_adapter_plus_reference import plus_state_dict
    root = str(tmp_path)
    ch = (32, 64, 128, 128)
    kw = dict(sample_size=8, block_out_channels=ch, attention_head_dim=4, norm_num_groups=8, cross_attention_dim=64)
    u2 = init_random_weights_(p.UNet2DConditionModel(**kw), seed=1)
    u2.save_pretrained(os.path.join(root, "sd", "unet"))
    init_random_weights_(p.AutoencoderKL(block_out_channels=(32, 64, 64, 64), norm_num_groups=8), seed=2) \
        .save_pretrained(os.path.join(root, "sd", "vae"))
    p.DDIMScheduler().save_pretrained(os.path.join(root, "sd", "scheduler"))
    init_random_weights_(p.MotionAdapter(block_out_channels=ch, motion_num_attention_heads=4, motion_norm_num_groups=8),
                         seed=3).save_pretrained(os.path.join(root, "motion"))
    init_random_weights_(p.I2VAdapterModule(2, ch, 4), seed=4).save_pretrained(
        os.path.join(root, "checkpoint", "demo", "epoch_3", "i2v_adapter"))
    probe = p.UNetMotionCrossFrameAttnModel.from_unet2d(u2, p.MotionAdapter(block_out_channels=ch, motion_num_attention_heads=4,
                                                                            motion_norm_num_groups=8), load_weights=False)
    os.makedirs(os.path.join(root, "ip", "models"))
    torch.save(plus_state_dict(probe, embed_dims=64, hidden=128, heads=2, depth=1, num_queries=16),
               os.path.join(root, "ip", "models", "ip-adapter-plus_sd15.bin"))
    vis = dict(hidden_size=64, intermediate_size=64, projection_dim=48, num_hidden_layers=2, num_attention_heads=1, num_channels=3,
               image_size=224, patch_size=14, hidden_act="gelu", layer_norm_eps=1e-5)
    enc = p.CLIPVisionModelWithProjection(**vis)
    enc.load_state_dict(seeded_state(vis, seed=6, qk_gain=3.0))
    enc.half().save_pretrained(os.path.join(root, "ip", "models", "image_encoder"))
    os.makedirs(os.path.join(root, "data", "images"))
    rs = np.random.RandomState(0)
    names = ["a cat on a boat", "two dogs, running"]
    with open(os.path.join(root, "data", "eval.csv"), "w") as f:
        f.write("image_path,name\n")
        for i, nm in enumerate(names):
            PIL.Image.fromarray((rs.rand(70, 90, 3) * 255).astype("uint8")).save(os.path.join(root, "data", "images", f"{i}.png"))
            f.write(f'images/{i}.png,"{nm}"\n')
    g = torch.Generator().manual_seed(5)
    save_file({"prompt_embeds": torch.randn(2, 7, 64, generator=g), "negative_prompt_embeds": torch.randn(1, 7, 64, generator=g)},
              os.path.join(root, "embeds.safetensors"))
    seen = []
    encode_image = I2VAdapterPipeline.encode_image

    def spy(self, image, *a, **k):
        out = encode_image(self, image, *a, **k)
        seen.append((tuple(out[0].shape), tuple(out[1].shape), type(self.unet.encoder_hid_proj).__name__,
                     sorted({(m.ip_num_tokens, m.ip_scale) for m in self.unet._cross_attention_layers()})))
        return out
    monkeypatch.setattr(I2VAdapterPipeline, "encode_image", spy)
    common = ["--task_name", "demo", "--checkpoint_epoch", "3", "--eval_data_path", os.path.join(root, "data", "eval.csv"),
              "--embeds", os.path.join(root, "embeds.safetensors"), "--model_path", os.path.join(root, "sd"),
              "--motion_adapter_path", os.path.join(root, "motion"), "--ip_adapter_path", os.path.join(root, "ip"),
              "--checkpoint_root", os.path.join(root, "checkpoint"), "--samples_root", os.path.join(root, "samples"),
              "--num_frames", "4", "--num_inference_steps", "4"]
    assert main(common + ["--ip_adapter", "--ip_adapter_weight_name", "ip-adapter-plus_sd15.bin", "--ip_adapter_scale", "0.5"]) == 0
    assert seen == [((1, 257, 64), (1, 257, 64), "Resampler", [(16, 0.5)])] * 2
    for nm in names:
        gif = PIL.Image.open(os.path.join(root, "samples", "demo", "epoch_3", f"{nm}.gif"))
        assert gif.n_frames == 4 and gif.size == (64, 64)
