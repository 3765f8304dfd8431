"""CPU: the load-time work and the refusals of clip_vision.CLIPVisionTower (no GPU, no kernel call): the flattened and padded patch weight
against torch's strided convolution in float64, the stacked q | k | v projection against the three separate ones, every configuration the
kernels do not take refused by name with its value, and the safetensors reader selecting exactly the vision tensors."""
import warnings

import pytest
import torch

from sd_standins import tiny_clip


def make_clip(hidden=128, heads=2, inter=256, layers=2, image=56, patch=14, proj=64, act='quick_gelu', seed=0):
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        from transformers import CLIPConfig, CLIPModel, CLIPTextConfig, CLIPVisionConfig
        tc = CLIPTextConfig(vocab_size=1000, hidden_size=32, intermediate_size=64, num_hidden_layers=1, num_attention_heads=2,
                            max_position_embeddings=77, projection_dim=proj, bos_token_id=998, eos_token_id=999, pad_token_id=999)
        vc = CLIPVisionConfig(hidden_size=hidden, intermediate_size=inter, num_hidden_layers=layers, num_attention_heads=heads,
                              image_size=image, patch_size=patch, projection_dim=proj, hidden_act=act)
        torch.manual_seed(seed)
        return CLIPModel(CLIPConfig(text_config=tc.to_dict(), vision_config=vc.to_dict(), projection_dim=proj)).eval()


@pytest.mark.parametrize('patch,size', [(14, 56), (32, 64), (16, 48)])
def test_patch_weight_matrix_is_the_strided_convolution(patch, size):
    from diffusion_tts_amd import clip_vision as cv, ops
    g = torch.Generator().manual_seed(patch)
    hidden, n = 24, 2
    w = torch.randn(hidden, 3, patch, patch, generator=g, dtype=torch.float64)
    x = torch.randn(n, 3, size, size, generator=g, dtype=torch.float64)
    kpad = ops.patch_kpad(patch)
    assert kpad % 64 == 0 and 0 <= kpad - 3 * patch * patch < 64
    assert (ops.patch_kpad(14), ops.patch_kpad(32)) == (640, 3072)
    wm = cv.patch_weight_matrix(w)
    assert tuple(wm.shape) == (hidden, kpad) and not wm[:, 3 * patch * patch:].any()
    rows = torch.nn.functional.unfold(x, patch, stride=patch).transpose(1, 2)             # [n, g*g, 3*p*p], columns in (c, py, px) order
    rows = torch.cat([rows, torch.zeros(n, rows.shape[1], kpad - rows.shape[2], dtype=torch.float64)], 2)
    got = rows @ wm.T                                                                      # [n, g*g, hidden]
    ref = torch.nn.functional.conv2d(x, w, stride=patch).flatten(2).transpose(1, 2)
    assert float((got - ref).abs().max()) <= 1e-12 * float(ref.abs().max())
    # the column of the documented formula holds the documented pixel
    c, py, px, gy, gx = 2, patch - 1, 3, 1, size // patch - 1
    assert rows[1, gy * (size // patch) + gx, (c * patch + py) * patch + px] == x[1, c, gy * patch + py, gx * patch + px]


def test_stacked_qkv_equals_the_three_projections():
    from diffusion_tts_amd import clip_vision as cv
    model = make_clip().requires_grad_(False)
    sd = model.state_dict()
    key = 'vision_model.encoder.layers.1.self_attn'
    w, b = cv.stack_qkv(sd, key)
    C = 128
    assert tuple(w.shape) == (3 * C, C) and tuple(b.shape) == (3 * C,)
    x = torch.randn(5, C, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    y = x @ w.double().T + b.double()
    att = model.vision_model.encoder.layers[1].self_attn
    for i, lin in enumerate((att.q_proj, att.k_proj, att.v_proj)):
        assert torch.equal(w[i * C:(i + 1) * C], lin.weight) and torch.equal(b[i * C:(i + 1) * C], lin.bias)
        ref = x @ lin.weight.double().T + lin.bias.double()
        assert float((y[:, i * C:(i + 1) * C] - ref).abs().max()) <= 1e-13 * float(ref.abs().max())
    assert abs((C // 2) ** -0.5 - att.scale) < 1e-15                                        # scale = head_dim ** -0.5, as transformers'


GOOD = dict(hidden_size=128, num_attention_heads=2, intermediate_size=256, image_size=56, patch_size=14, hidden_act='quick_gelu',
            dtype=torch.float16)


@pytest.mark.parametrize('change,names', [
    (dict(hidden_size=96, num_attention_heads=1), ['hidden_size=96', 'head dim 96']),
    (dict(hidden_size=4096, num_attention_heads=16), ['hidden_size=4096']),
    (dict(num_attention_heads=4), ['head dim 32']),
    (dict(num_attention_heads=3), ['head dim 42.6667']),
    (dict(hidden_size=1024, num_attention_heads=2), ['head dim 512']),
    (dict(intermediate_size=200), ['intermediate_size=200']),
    (dict(image_size=60), ['image_size=60', 'patch_size=14']),
    (dict(hidden_act='gelu_new'), ["hidden_act='gelu_new'"]),
    (dict(dtype=torch.float32), ['dtype=torch.float32']),
    (dict(dtype='f16x3'), ['dtype=f16x3']),
])
def test_refusals_name_the_offending_value(change, names):
    from diffusion_tts_amd import clip_vision as cv
    cv.check_config(**GOOD)
    cv.check_config(**dict(GOOD, hidden_act='gelu', dtype=torch.bfloat16, hidden_size=2048, num_attention_heads=8))
    with pytest.raises(ValueError) as e:
        cv.check_config(**dict(GOOD, **change))
    for name in names:
        assert name in str(e.value), (name, str(e.value))
    # the constructor refuses the same way, before it needs a GPU or looks at a parameter
    kw = dict(GOOD, **change)
    with pytest.raises(ValueError) as e2:
        cv.CLIPVisionTower({}, num_hidden_layers=2, **kw)
    assert str(e2.value) == str(e.value)


def test_the_stock_tiny_clip_is_refused_for_its_head_dim():
    from diffusion_tts_amd import clip_vision as cv
    with pytest.raises(ValueError) as e:
        cv.CLIPVisionTower.from_clip_model(tiny_clip())
    assert 'head dim 16' in str(e.value) and 'hidden_size=32' in str(e.value)
    from diffusion_tts_amd.scorers import CLIPScorer
    with pytest.raises(ValueError, match='vision_tower'):
        CLIPScorer(model=tiny_clip(), device='cpu', device_preprocess=False, vision_tower='rocm')
    with pytest.raises(ValueError, match='head dim 16'):                                    # no fallback to the transformers tower
        CLIPScorer(model=tiny_clip(), device='cpu', device_preprocess=False, vision_tower='hip')


def test_from_pretrained_reads_exactly_the_vision_tensors(tmp_path):
    from diffusion_tts_amd import clip_vision as cv
    model = make_clip(act='gelu', image=28, layers=1)
    model.save_pretrained(str(tmp_path), safe_serialization=True)
    cfg, sd = cv.read_vision_tensors(str(tmp_path))
    full = model.state_dict()
    want = {k for k in full if k.startswith('vision_model.') or k == 'visual_projection.weight'}
    assert set(sd) == want and len(want) == 8 + 16
    assert not any('text' in k or k == 'logit_scale' for k in sd)
    for k in want:
        assert torch.equal(sd[k], full[k]), k
    assert cfg == dict(hidden_size=128, intermediate_size=256, num_hidden_layers=1, num_attention_heads=2, image_size=28, patch_size=14,
                       hidden_act='gelu', layer_norm_eps=1e-5, projection_dim=64)
    with pytest.raises(FileNotFoundError, match='config.json'):
        cv.read_vision_tensors(str(tmp_path / 'nothing'))


def test_main_parses_the_clip_tower_flag():
    import main
    p = main.build_parser()
    base = ['--backend', 'sd', '--scorer', 'clip']
    assert p.parse_args(base).clip_tower == 'transformers'
    assert p.parse_args(base + ['--clip-tower', 'hip']).clip_tower == 'hip'
    with pytest.raises(SystemExit):
        p.parse_args(base + ['--clip-tower', 'triton'])
