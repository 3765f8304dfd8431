"""CPU: the interface of the split-precision (ops.F16X3) CLIP text tower, clip_text.CLIPTextTowerX3 -- its configuration check
(check_config_x3, a function of its own: clip_text.check_config keeps refusing 'f16x3' and keeps not knowing `split_precision`, pinned by
tests/test_clip_vision_x3_cpu.py), the scorer's text_tower_dtype keyword, the two command-line flags, and the host refusals of the two new
ops.  No GPU, no kernel call."""
import warnings

import pytest
import torch

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


def test_check_config_x3_takes_the_clip_text_widths_and_names_what_it_refuses():
    from diffusion_tts_amd import clip_text as ct, ops
    assert issubclass(ct.CLIPTextTowerX3, ct.CLIPTextTower) and ct.CLIPTextTowerX3.DEFAULT_DTYPE == ops.F16X3
    assert ct.CLIPTextTower.DEFAULT_DTYPE == torch.float16
    for hidden, heads, inter in ((512, 8, 2048), (768, 12, 3072), (1024, 16, 4096)):
        ct.check_config_x3(hidden, heads, inter, 'quick_gelu', ops.F16X3)
    ct.check_config_x3(dtype=ops.F16X3, **dict(GOOD_TEXT, hidden_act='gelu'), projection_dim=64)
    with pytest.raises(ValueError) as e:                                  # head dim 32: the text settings of the other GPU tests
        ct.check_config_x3(dtype=ops.F16X3, **dict(GOOD_TEXT, num_attention_heads=4))
    assert 'head dim 32' in str(e.value) and "dts_attention_x3_masked's 64" in str(e.value) and 'dtype' not in str(e.value)
    with pytest.raises(ValueError, match='head dim 128'):
        ct.check_config_x3(dtype=ops.F16X3, **dict(GOOD_TEXT, num_attention_heads=1))
    for bad, name in ((torch.float16, 'dtype=torch.float16'), (torch.bfloat16, 'dtype=torch.bfloat16'), (torch.float32, 'dtype=torch.float32')):
        with pytest.raises(ValueError) as e:
            ct.check_config_x3(dtype=bad, **GOOD_TEXT)
        assert name in str(e.value) and str(e.value).startswith('CLIPTextTower: ')
        with pytest.raises(ValueError) as e2:                             # refused before a GPU or a parameter is looked at
            ct.CLIPTextTowerX3({}, num_hidden_layers=2, dtype=bad, **GOOD_TEXT)
        assert str(e2.value) == str(e.value)
    with pytest.raises(ValueError) as e:
        ct.check_config_x3(dtype=torch.float32, **GOOD_TEXT)
    assert 'there is no float32 form of this tower' in str(e.value)
    with pytest.raises(ValueError) as e:
        ct.check_config_x3(dtype=ops.F16X3, **dict(GOOD_TEXT, hidden_act='gelu_new'))
    assert "hidden_act='gelu_new'" in str(e.value)
    with pytest.raises(ValueError, match='vocab_size=0'):
        ct.check_config_x3(dtype=ops.F16X3, vocab_size=0, **GOOD_TEXT)
    with pytest.raises(ValueError, match="hidden_act='relu'"):
        ct.CLIPTextTowerX3({}, num_hidden_layers=2, **dict(GOOD_TEXT, hidden_act='relu'))


def test_the_scorer_takes_text_tower_dtype_and_builds_no_tower_for_transformers():
    from diffusion_tts_amd import ops
    from diffusion_tts_amd.scorers import CLIPScorer
    model = small_clip()
    for bad in (torch.float32, 'f32', 'f16', 16):
        with pytest.raises(ValueError) as e:
            CLIPScorer(model=model, device='cpu', device_preprocess=False, text_tower_dtype=bad)
        assert 'text_tower_dtype' in str(e.value) and repr(bad) in str(e.value)
    for ok in (None, torch.float16, torch.bfloat16, ops.F16X3):
        s = CLIPScorer(model=model, device='cpu', device_preprocess=False, text_tower_dtype=ok)
        assert s.text_tower == 'transformers' and s._text_tower is None and s._tower is None
    # the refusal of tower_dtype='f16x3' alone now says where the split-precision text tower is asked for
    with pytest.raises(ValueError) as e:
        CLIPScorer(model=model, device='cpu', device_preprocess=False, text_tower='hip', tower_dtype=ops.F16X3)
    assert "text_tower_dtype='f16x3'" in str(e.value) and 'no split-precision form' in str(e.value)
    # asked for, it is the tower's own refusal that is met on a machine without a GPU, not the scorer's
    with pytest.raises((RuntimeError, ValueError)) as e:
        CLIPScorer(model=model, device='cpu', device_preprocess=False, text_tower='hip', tower_dtype=ops.F16X3, text_tower_dtype=ops.F16X3,
                   vision_tower='transformers')
    assert 'no split-precision form' not in str(e.value)


def test_main_lists_the_two_clip_text_tower_flags_with_their_defaults():
    import main
    p = main.build_parser()
    text = ' '.join(p.format_help().split())
    assert '--clip-text-tower {transformers,hip}' in text and '--clip-text-tower-dtype {f16,bf16,f16x3}' in text
    base = ['--backend', 'sd', '--scorer', 'clip']
    a = p.parse_args(base)
    assert a.clip_text_tower == 'transformers' and a.clip_text_tower_dtype is None
    assert p.get_default('clip_text_tower') == 'transformers' and p.get_default('clip_text_tower_dtype') is None
    a = p.parse_args(base + ['--clip-text-tower', 'hip', '--clip-text-tower-dtype', 'f16x3'])
    assert a.clip_text_tower == 'hip' and a.clip_text_tower_dtype == 'f16x3'
    with pytest.raises(SystemExit):
        p.parse_args(base + ['--clip-text-tower-dtype', 'f32'])
    with pytest.raises(SystemExit):
        p.parse_args(base + ['--clip-text-tower', 'diffusers'])
    assert '--clip-text-tower' in main.__doc__ and '--clip-text-tower-dtype' in main.__doc__


def test_get_scorer_passes_both_flags_to_the_scorer():
    import main
    from diffusion_tts_amd import ops
    model = small_clip()
    s = main.get_scorer('sd', 'clip', 'cpu', clip_model=model, clip_text_tower='transformers', clip_text_tower_dtype='f16x3')
    assert s.text_tower == 'transformers' and s._text_tower is None
    with pytest.raises(ValueError, match="text_tower_dtype='f16x3'"):     # the pinned refusal, reached through main's keywords
        main.get_scorer('sd', 'clip', 'cpu', clip_model=model, clip_tower_dtype='f16x3', clip_text_tower='hip')
    assert ops.F16X3 == main.CLIP_TOWER_DTYPES['f16x3']


def test_the_new_ops_refuse_on_the_host_before_any_launch():
    from diffusion_tts_amd import ops
    c = 3 * 2 * 64
    x16 = torch.zeros(2, 5, c, dtype=torch.float16)
    with pytest.raises(ValueError, match=r'attention_x3_masked: qkv must be float32 .*torch.float16'):
        ops.attention_x3_masked(x16, 2, 0.125)
    with pytest.raises(ValueError, match=r'attention_x3_masked: qkv \(2, 5, 384\) is not \[n, t, 3 \* 5 heads \* d\]'):
        ops.attention_x3_masked(x16.float(), 5, 0.125)
    with pytest.raises(ValueError, match='attention_x3_masked: qkv'):
        ops.attention_x3_masked(x16.float().view(10, c), 2, 0.125)
    with pytest.raises(ValueError, match=r'attention_x3_masked: key_len \(3,\) torch.int32 is not int32 \[2\]'):
        ops.attention_x3_masked(x16.float(), 2, 0.125, key_len=torch.ones(3, dtype=torch.int32))
    with pytest.raises(ValueError, match=r'attention_x3_masked: key_len \(2,\) torch.int64 is not int32 \[2\]'):
        ops.attention_x3_masked(x16.float(), 2, 0.125, key_len=torch.ones(2, dtype=torch.int64))
    tok, pos = torch.zeros(10, 64), torch.zeros(7, 64)
    with pytest.raises(ValueError, match=r'text_tokens_f32: token id 10 is outside \[0, 10\)'):
        ops.text_tokens_f32(torch.tensor([[1, 10]]), tok, pos)
    with pytest.raises(ValueError, match=r'text_tokens_f32: token id -1 is outside'):
        ops.text_tokens_f32(torch.tensor([[-1, 2]]), tok, pos)
    with pytest.raises(ValueError, match='text_tokens_f32: ids must be an integer tensor'):
        ops.text_tokens_f32(torch.zeros(1, 2), tok, pos)
    with pytest.raises(ValueError, match='text_tokens_f32: tok'):
        ops.text_tokens_f32(torch.zeros(1, 8, dtype=torch.long), tok, pos)           # more tokens than positions
    with pytest.raises(ValueError, match='text_tokens_f32: 60 channels'):
        ops.text_tokens_f32(torch.zeros(1, 2, dtype=torch.long), torch.zeros(10, 60), torch.zeros(7, 60))
