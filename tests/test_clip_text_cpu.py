"""CPU: the host side of clip_text.CLIPTextTower (no GPU, no kernel call): the pooled positions against transformers under both eos rules,
the attention mask -> key length conversion and its refusals, every configuration the kernels do not take refused by name with its value,
the safetensors reader selecting exactly the text tensors, state-dict mismatches named, and the `--text-encoder` flag."""
import json
import warnings

import pytest
import torch


def text_config(hidden=128, heads=2, inter=256, layers=2, vocab=1000, eos=999, proj=64, act='quick_gelu'):
    from transformers import CLIPTextConfig
    return CLIPTextConfig(vocab_size=vocab, hidden_size=hidden, intermediate_size=inter, num_hidden_layers=layers, num_attention_heads=heads,
                          max_position_embeddings=77, projection_dim=proj, bos_token_id=998, eos_token_id=eos, pad_token_id=999,
                          hidden_act=act)


def make_text(seed=1234, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        from transformers import CLIPTextModelWithProjection
        torch.manual_seed(seed)
        return CLIPTextModelWithProjection(text_config(**kw)).eval()


def make_clip(seed=0, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        from transformers import CLIPConfig, CLIPModel, CLIPVisionConfig
        vc = CLIPVisionConfig(hidden_size=32, intermediate_size=64, num_hidden_layers=1, num_attention_heads=2, image_size=28, patch_size=14,
                              projection_dim=48)
        torch.manual_seed(seed)
        return CLIPModel(CLIPConfig(text_config=text_config(proj=48, **kw).to_dict(), vision_config=vc.to_dict(), projection_dim=48)).eval()


def ids_77_9_40():
    """three rows of 77 ids, bos first, lengths 77 / 9 / 40, the end token 999 (the largest id) at len - 1 and as padding after it"""
    ids = torch.randint(0, 998, (3, 77), generator=torch.Generator().manual_seed(5))
    ids[:, 0] = 998
    for b, n in enumerate((77, 9, 40)):
        ids[b, n - 1:] = 999
    return ids


@pytest.mark.parametrize('eos', [999, 2])
def test_pooled_positions_are_transformers(eos):
    """last_hidden_state[arange, pos] == pooler_output of the float32 module, under the first-eos rule and the legacy argmax rule"""
    from diffusion_tts_amd.clip_text import pooled_positions
    model = make_text(eos=eos, layers=1)
    ids = ids_77_9_40()
    pos = pooled_positions(ids, eos)
    assert pos.dtype == torch.int64 and pos.tolist() == [76, 8, 39]
    with torch.no_grad():
        out = model.text_model(input_ids=ids)
    assert torch.equal(out.last_hidden_state[torch.arange(3), pos], out.pooler_output)
    # the two rules differ where they should: an id above the eos id earlier in the row moves only the argmax rule
    ids2 = torch.tensor([[5, 7, 3, 6, 3, 3]])
    assert pooled_positions(ids2, 3).tolist() == [2] and pooled_positions(ids2, 2).tolist() == [1]
    assert pooled_positions(ids2, 900).tolist() == [0]                 # no eos in the row: transformers' argmax of an all-false row
    with pytest.raises(ValueError, match='pooled_positions'):
        pooled_positions(ids2[0], 3)


def test_mask_to_key_len_and_its_refusals():
    from diffusion_tts_amd.clip_text import mask_key_len
    assert mask_key_len(None, 2, 4) is None
    assert mask_key_len(torch.ones(2, 4, dtype=torch.long), 2, 4) is None              # all ones: nothing to hide
    kl = mask_key_len(torch.tensor([[1, 1, 1, 1], [1, 0, 0, 0], [1, 1, 1, 0]]), 3, 4)
    assert kl.dtype == torch.int32 and kl.tolist() == [4, 1, 3]
    assert mask_key_len(torch.tensor([[True, True, False]]), 1, 3).tolist() == [2]
    for bad, words in (([[1, 1, 1], [0, 1, 1]], 'row 1 is left-padded'), ([[1, 0, 1], [1, 1, 1]], 'row 0 has a hole'),
                       ([[1, 1, 1], [0, 0, 0]], 'row 1 is all zero'), ([[1, 2, 0], [1, 1, 1]], 'other than 0 and 1')):
        with pytest.raises(ValueError, match=words):
            mask_key_len(torch.tensor(bad), 2, 3)
    with pytest.raises(ValueError, match=r'attention_mask \(2, 3\) does not match input_ids \(2, 4\)'):
        mask_key_len(torch.ones(2, 3), 2, 4)


GOOD = dict(hidden_size=128, num_attention_heads=2, intermediate_size=256, hidden_act='quick_gelu', dtype=torch.float16)


@pytest.mark.parametrize('change,names', [
    (dict(hidden_size=64, num_attention_heads=2), ['head dim 32', 'hidden_size=64', 'num_attention_heads=2']),
    (dict(hidden_size=96, num_attention_heads=1), ['hidden_size=96', 'head dim 96']),
    (dict(hidden_size=4096, num_attention_heads=64), ['hidden_size=4096']),
    (dict(hidden_size=256, num_attention_heads=2), ['head dim 128']),
    (dict(intermediate_size=200), ['intermediate_size=200']),
    (dict(dtype=torch.float32), ['dtype=torch.float32']),
    (dict(dtype='f16x3'), ['dtype=f16x3']),
    (dict(hidden_act='relu'), ["hidden_act='relu'"]),
])
def test_refusals_name_the_offending_value(change, names):
    from diffusion_tts_amd import clip_text as ct
    ct.check_config(**GOOD)
    ct.check_config(**dict(GOOD, hidden_act='gelu', dtype=torch.bfloat16, hidden_size=1280, num_attention_heads=20, intermediate_size=5120))
    with pytest.raises(ValueError) as e:
        ct.check_config(**dict(GOOD, **change))
    for name in names:
        assert name in str(e.value), (name, str(e.value))
    # the constructor refuses the same way, before it needs a GPU or looks at a parameter
    with pytest.raises(ValueError) as e2:
        ct.CLIPTextTower({}, num_hidden_layers=2, **dict(GOOD, **change))
    assert str(e2.value) == str(e.value)


def test_construction_without_a_gpu_says_so(monkeypatch):
    from diffusion_tts_amd.clip_text import CLIPTextTower
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    with pytest.raises(RuntimeError, match='needs a GPU'):
        CLIPTextTower.from_text_model(make_text(layers=1))
    from diffusion_tts_amd.scorers import CLIPScorer
    from sd_standins import tiny_clip
    with pytest.raises(ValueError, match='text_tower'):
        CLIPScorer(model=tiny_clip(), device='cpu', device_preprocess=False, text_tower='rocm')
    with pytest.raises(ValueError, match='head dim 16'):                                    # no fallback to the transformers tower
        CLIPScorer(model=tiny_clip(), device='cpu', device_preprocess=False, text_tower='hip')


def test_from_pretrained_reads_exactly_the_text_tensors(tmp_path):
    from diffusion_tts_amd import clip_text as ct
    model = make_clip(layers=1, act='gelu', inter=192)
    model.save_pretrained(str(tmp_path), safe_serialization=True)
    cfg, sd = ct.read_text_tensors(str(tmp_path))
    full = model.state_dict()
    want = {k for k in full if k.startswith('text_model.') or k == 'text_projection.weight'}
    assert set(sd) == want and len(want) == 2 + 2 + 16 + 1              # embeddings, final norm, one layer, projection
    assert not any('vision' in k or 'visual' in k or k == 'logit_scale' for k in sd)
    for k in want:
        assert torch.equal(sd[k], full[k]), k
    # the nested text_config is honoured (the top-level dict holds none of these), projection_dim is the CLIPModel's own
    assert cfg == dict(vocab_size=1000, hidden_size=128, intermediate_size=192, num_hidden_layers=1, num_attention_heads=2,
                       max_position_embeddings=77, hidden_act='gelu', layer_norm_eps=1e-5, eos_token_id=999, projection_dim=48)
    with pytest.raises(FileNotFoundError, match='config.json'):
        ct.read_text_tensors(str(tmp_path / 'nothing'))


def test_config_defaults_and_bare_key_names(tmp_path):
    """absent keys take CLIPTextConfig's defaults; a text model stored without the `text_model.` prefix is read under it"""
    from safetensors.torch import save_file
    from transformers import CLIPTextConfig
    from diffusion_tts_amd import clip_text as ct
    d = CLIPTextConfig().to_dict()
    assert ct.text_config({}) == {k: d[k] for k in ct.CONFIG_DEFAULTS}
    assert ct.text_config({'text_config': {'hidden_size': 768}, 'projection_dim': 640})['projection_dim'] == 640
    assert ct.text_config({'text_config': {'hidden_size': 768}, 'projection_dim': 640})['hidden_size'] == 768
    full = make_text(layers=1).state_dict()
    bare = {k[len('text_model.'):]: v.contiguous() for k, v in full.items() if k.startswith('text_model.')}
    save_file(bare, str(tmp_path / 'model.safetensors'))
    (tmp_path / 'config.json').write_text(json.dumps({'hidden_size': 128, 'num_attention_heads': 2}))
    cfg, sd = ct.read_text_tensors(str(tmp_path))
    assert set(sd) == {k for k in full if k.startswith('text_model.')} and cfg['hidden_size'] == 128 and cfg['vocab_size'] == 49408
    assert torch.equal(sd['text_model.final_layer_norm.weight'], full['text_model.final_layer_norm.weight'])


def test_state_dict_mismatches_are_named(monkeypatch):
    """a state dict that is not the configuration's is named by _check_shapes, which runs before any device work"""
    from diffusion_tts_amd import clip_text as ct
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: True)       # past the "needs a GPU" error; the refusals below come before a kernel
    sd = dict(make_text().state_dict())
    kw = dict(vocab_size=1000, hidden_size=128, num_attention_heads=2, intermediate_size=256, max_position_embeddings=77, num_hidden_layers=2)
    build = lambda **over: ct.CLIPTextTower(sd, **dict(kw, **over))
    with pytest.raises(ValueError, match=r"token_embedding.weight has shape \(1000, 128\), but vocab_size=2000"):
        build(vocab_size=2000)
    with pytest.raises(ValueError, match=r'mlp.fc1.weight has shape \(256, 128\).*intermediate_size=512'):
        build(intermediate_size=512)
    with pytest.raises(ValueError, match='more than num_hidden_layers=1 layers'):
        build(num_hidden_layers=1)
    with pytest.raises(ValueError, match=r"no 'text_model.encoder.layers.2.self_attn.q_proj.weight' \(num_hidden_layers=3\)"):
        build(num_hidden_layers=3)
    with pytest.raises(ValueError, match=r'text_projection.weight has shape \(64, 128\).*projection_dim=32'):
        build(projection_dim=32)
    with pytest.raises(ValueError, match=r"projection_dim=64, but the state dict has no 'text_projection.weight'"):
        ct.CLIPTextTower({k: v for k, v in sd.items() if k != 'text_projection.weight'}, projection_dim=64, **kw)


def test_main_parses_the_text_encoder_flag(monkeypatch, tmp_path):
    import main
    p = main.build_parser()
    base = ['--backend', 'sd', '--scorer', 'brightness']
    assert p.parse_args(base).text_encoder == 'transformers'
    assert p.parse_args(base + ['--text-encoder', 'hip']).text_encoder == 'hip'
    with pytest.raises(SystemExit):
        p.parse_args(base + ['--text-encoder', 'triton'])
    monkeypatch.setenv('DTS_SD_TEXT_ENCODER_DIR', str(tmp_path / 'nothing'))                # a missing directory is an error, not a fallback
    with pytest.raises(FileNotFoundError, match='DTS_SD_TEXT_ENCODER_DIR'):
        main.load_sd_text_encoder('runwayml/stable-diffusion-v1-5', torch.device('cpu'), 'hip')
