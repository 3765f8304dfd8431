"""CPU: the interface of the split-precision (ops.F16X3) CLIP image tower, clip_vision.CLIPVisionTowerX3 -- which towers take the mode, which refusals stay, and the
command-line flag.  No GPU, no kernel call."""
import warnings

import pytest
import torch

GOOD_VISION = dict(hidden_size=128, num_attention_heads=2, intermediate_size=256, image_size=56, patch_size=14, hidden_act='quick_gelu')
GOOD_TEXT = dict(hidden_size=128, num_attention_heads=2, intermediate_size=256, hidden_act='quick_gelu')


def small_clip():
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        from transformers import CLIPConfig, CLIPModel, CLIPTextConfig, CLIPVisionConfig
        tc = CLIPTextConfig(vocab_size=300, hidden_size=64, intermediate_size=128, num_hidden_layers=1, num_attention_heads=1,
                            max_position_embeddings=77, projection_dim=32, bos_token_id=298, eos_token_id=299, pad_token_id=299)
        vc = CLIPVisionConfig(hidden_size=64, intermediate_size=128, num_hidden_layers=1, num_attention_heads=1, image_size=28, patch_size=14,
                              projection_dim=32)
        torch.manual_seed(0)
        return CLIPModel(CLIPConfig(text_config=tc.to_dict(), vision_config=vc.to_dict(), projection_dim=32)).eval()


def test_the_vision_tower_takes_f16x3_and_the_text_tower_does_not():
    """the split-precision mode is a class of its own, CLIPVisionTowerX3, with a check of its own (check_config(split_precision=True)):
    CLIPVisionTower's refusal of every dtype but float16 / bfloat16 -- 'f16x3' included -- is pinned by tests/test_clip_vision_cpu.py and stays"""
    from diffusion_tts_amd import clip_text as ct, clip_vision as cv, ops
    assert ops.F16X3 == 'f16x3'
    assert issubclass(cv.CLIPVisionTowerX3, cv.CLIPVisionTower) and cv.CLIPVisionTowerX3.DEFAULT_DTYPE == ops.F16X3
    x3 = dict(dtype=ops.F16X3, split_precision=True)
    cv.check_config(**x3, **GOOD_VISION)
    cv.check_config(**x3, **dict(GOOD_VISION, hidden_size=1024, num_attention_heads=16, intermediate_size=4096, image_size=224))
    cv.check_config(**x3, **dict(GOOD_VISION, hidden_size=256, num_attention_heads=1, hidden_act='gelu'))       # head dim 256
    with pytest.raises(ValueError) as e:
        ct.check_config(dtype=ops.F16X3, **GOOD_TEXT)
    assert 'dtype=f16x3' in str(e.value)
    with pytest.raises(TypeError):                                        # the text tower has no such form to ask for
        ct.check_config(dtype=ops.F16X3, split_precision=True, **GOOD_TEXT)
    with pytest.raises(ValueError) as e:                                  # the 16-bit tower's own refusal, unchanged
        cv.check_config(dtype=ops.F16X3, **GOOD_VISION)
    assert 'dtype=f16x3' in str(e.value)
    # the mode changes nothing else of what the vision tower refuses
    with pytest.raises(ValueError) as e:
        cv.check_config(**x3, **dict(GOOD_VISION, num_attention_heads=4, hidden_act='gelu_new'))
    assert 'head dim 32' in str(e.value) and "hidden_act='gelu_new'" in str(e.value) and 'dtype' not in str(e.value)
    # and the split-precision tower has one dtype: the 16-bit ones are the other class's; refused before a GPU or a parameter is looked at
    for bad, name in ((torch.float16, 'dtype=torch.float16'), ('f32x3', 'dtype=f32x3')):
        with pytest.raises(ValueError) as e:
            cv.check_config(dtype=bad, split_precision=True, **GOOD_VISION)
        assert name in str(e.value)
        with pytest.raises(ValueError) as e2:
            cv.CLIPVisionTowerX3({}, num_hidden_layers=2, dtype=bad, **GOOD_VISION)
        assert str(e2.value) == str(e.value)


def test_float32_stays_refused_by_both_towers():
    from diffusion_tts_amd import clip_text as ct, clip_vision as cv
    import functools
    for check, good in ((cv.check_config, GOOD_VISION), (functools.partial(cv.check_config, split_precision=True), GOOD_VISION),
                        (ct.check_config, GOOD_TEXT)):
        with pytest.raises(ValueError) as e:
            check(dtype=torch.float32, **good)
        assert 'dtype=torch.float32' in str(e.value) and 'there is no float32 form of this tower' in str(e.value)
    with pytest.raises(ValueError, match='dtype=torch.float32'):
        cv.CLIPVisionTowerX3({}, num_hidden_layers=2, dtype=torch.float32, **GOOD_VISION)


def test_the_scorer_refuses_a_split_precision_text_tower_by_name():
    from diffusion_tts_amd import ops
    from diffusion_tts_amd.scorers import CLIPScorer
    model = small_clip()
    with pytest.raises(ValueError) as e:
        CLIPScorer(model=model, device='cpu', device_preprocess=False, text_tower='hip', tower_dtype=ops.F16X3)
    assert "text_tower='hip'" in str(e.value) and 'f16x3' in str(e.value) and 'no split-precision form' in str(e.value)
    with pytest.raises(ValueError, match='no split-precision form'):        # whatever the image tower is
        CLIPScorer(model=model, device='cpu', device_preprocess=False, vision_tower='hip', text_tower='hip', tower_dtype=ops.F16X3)
    # tower_dtype alone selects nothing: the stock towers ignore it
    s = CLIPScorer(model=model, device='cpu', device_preprocess=False, tower_dtype=ops.F16X3)
    assert s._tower is None and s._text_tower is None


def test_main_lists_the_clip_tower_dtype_flag_with_default_f16():
    import main
    p = main.build_parser()
    text = p.format_help()
    assert '--clip-tower-dtype {f16,bf16,f16x3}' in text and 'f16 (default)' in ' '.join(text.split())
    base = ['--backend', 'sd', '--scorer', 'clip', '--clip-tower', 'hip']
    assert p.parse_args(base).clip_tower_dtype == 'f16' and p.get_default('clip_tower_dtype') == 'f16'
    assert p.parse_args(base + ['--clip-tower-dtype', 'f16x3']).clip_tower_dtype == 'f16x3'
    with pytest.raises(SystemExit):
        p.parse_args(base + ['--clip-tower-dtype', 'f32'])
    from diffusion_tts_amd import ops
    assert main.CLIP_TOWER_DTYPES == {'f16': torch.float16, 'bf16': torch.bfloat16, 'f16x3': ops.F16X3}
    assert '--clip-tower-dtype' in main.__doc__


def test_the_split_precision_wrappers_refuse_on_the_host_by_name():
    """shape and dtype errors of the new ops are raised before any launch (and before the tensor's device is looked at)"""
    from diffusion_tts_amd import ops
    x16 = torch.zeros(2, 3, 1, 64, dtype=torch.float16)
    g = torch.ones(64)
    with pytest.raises(ValueError, match='layer_norm_x3: x must be a float32'):
        ops.layer_norm_x3(x16, g, g)
    with pytest.raises(ValueError, match='gelu_x3: x must be a float32'):
        ops.gelu_x3(x16)
    with pytest.raises(ValueError, match="gelu_x3: kind 'relu'"):
        ops.gelu_x3(x16.float(), 'relu')
    with pytest.raises(ValueError, match='patchify_x3: x must be a float32'):
        ops.patchify_x3(torch.zeros(1, 3, 28, 28, dtype=torch.float16), 14)
    with pytest.raises(ValueError, match='vit_tokens_f32: patches must be a float32'):
        ops.vit_tokens_f32(x16.view(2, 3, 64), g, torch.zeros(4, 64))
    with pytest.raises(ValueError, match='vit_head_f32: tokens must be a float32'):
        ops.vit_head_f32(x16.view(2, 3, 64), g, g)
