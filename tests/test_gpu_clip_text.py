"""GPU: dts_text_tokens, clip_text.CLIPTextTower, the tower as SDSearchPipeline's text encoder, CLIPScorer(text_tower='hip') and
`main.py --text-encoder hip`, against transformers itself -- the modules the reference calls.

The tower computes in float16 / bfloat16, so the yardstick is that of tests/test_gpu_clip_vision.py, the project's margin for 16-bit
modules: e32 = the transformers module in float32, e16 = the same module deep-copied to the tower's type, eh = the HIP tower;
max|eh - e32| <= 3 max|e16 - e32|, err_16 > 0, for `last_hidden_state` and `text_embeds` separately.  Random-init
CLIPTextModelWithProjection under torch.manual_seed(1234), projection_dim 64.  Ids: three rows of 77 random ids with bos first, row lengths
77 / 9 / 40, the end token at len - 1 and end-token padding after it; once without a mask and once with the right-padding mask, where ALL
rows are compared, the padded ones included.  The mask comparison has teeth only if the mask moves the padded rows by far more than the
yardstick: asserted from transformers alone, max|e32(masked) - e32(unmasked)| over the padded rows >= 10 * 3 * err_16."""
import copy
import os
import sys
import warnings

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = 'cuda'
DTYPES = [torch.float16, torch.bfloat16]
DTN = {torch.float16: 'f16', torch.bfloat16: 'bf16'}
# `eos` is the configuration's eos_token_id; `end` the id that ends a row.  Under the legacy rule (eos_token_id == 2) transformers pools at
# argmax(ids), so the end token must be the largest id, as in CLIP's vocabulary.
CONFIGS = {
    'w128': dict(hidden=128, heads=2, inter=256, layers=2, vocab=1000, eos=999, bos=998, end=999),
    'w128_legacy': dict(hidden=128, heads=2, inter=256, layers=2, vocab=1000, eos=2, bos=998, end=999),
    'L14x2': dict(hidden=768, heads=12, inter=3072, layers=2, vocab=49408, eos=49407, bos=49406, end=49407),   # SD-1.5 / ViT-L/14 text widths
}
LENS = (77, 9, 40)
POOLED = [76, 8, 39]
_MODELS = {}


def text_config(name):
    from transformers import CLIPTextConfig
    c = CONFIGS[name]
    return CLIPTextConfig(vocab_size=c['vocab'], hidden_size=c['hidden'], intermediate_size=c['inter'], num_hidden_layers=c['layers'],
                          num_attention_heads=c['heads'], max_position_embeddings=77, projection_dim=64, bos_token_id=c['bos'],
                          eos_token_id=c['eos'], pad_token_id=c['end'])


def text_model(name):
    if name not in _MODELS:
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            from transformers import CLIPTextModelWithProjection
            torch.manual_seed(1234)
            _MODELS[name] = CLIPTextModelWithProjection(text_config(name)).eval().to(DEV)
    return _MODELS[name]


def ids_and_mask(name, seed=5):
    c = CONFIGS[name]
    ids = torch.randint(0, c['bos'], (3, 77), generator=torch.Generator().manual_seed(seed))
    ids[:, 0] = c['bos']
    mask = torch.zeros(3, 77, dtype=torch.long)
    for b, n in enumerate(LENS):
        ids[b, n - 1:] = c['end']
        mask[b, :n] = 1
    return ids, mask


def reference(model, ids, mask):
    with torch.no_grad():
        out = model(input_ids=ids.to(DEV), attention_mask=None if mask is None else mask.to(DEV))
    return out.last_hidden_state.float(), out.text_embeds.float()


# ---- dts_text_tokens --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES, ids=lambda d: DTN[d])
@pytest.mark.parametrize('c', [64, 768])
@pytest.mark.parametrize('t', [1, 77])
def test_text_tokens_bit_equal(t, c, dtype):
    from diffusion_tts_amd import ops
    vocab, n = 1000, 3
    g = torch.Generator().manual_seed(100 * t + c)
    tok, pos = torch.randn(vocab, c, generator=g), torch.randn(77, c, generator=g)
    ids = torch.randint(0, vocab, (n, t), generator=g)
    ids[0, 0], ids[1, 0], ids[2, 0] = 0, vocab - 1, vocab - 1           # the two ends of the table, and a repeat
    if t > 2:
        ids[0, 1], ids[0, 2], ids[1, t - 1] = 7, 7, 0
    want = (tok[ids].float() + pos[:t].float()).to(dtype)
    tok_d, pos_d = tok.to(DEV), pos.to(DEV)
    got = ops.text_tokens(ids, tok_d, pos_d, dtype)
    assert got.dtype == dtype and tuple(got.shape) == (n, t, c) and torch.equal(got.cpu(), want)
    assert torch.equal(ops.text_tokens(ids.to(DEV).to(torch.int32), tok_d, pos_d, dtype), got)      # ids already on the device: copied back
    for bad in (vocab, -1):
        wrong = ids.clone()
        wrong[n - 1, t - 1] = bad
        with pytest.raises(ValueError, match=f'token id {bad} '):
            ops.text_tokens(wrong, tok_d, pos_d, dtype)


# ---- the tower against transformers -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES, ids=lambda d: DTN[d])
@pytest.mark.parametrize('name', list(CONFIGS))
def test_tower_against_transformers(name, dtype):
    from diffusion_tts_amd.clip_text import CLIPTextTower, pooled_positions
    model = text_model(name)
    m16 = copy.deepcopy(model).to(dtype)
    ids, mask = ids_and_mask(name)
    assert pooled_positions(ids, CONFIGS[name]['eos']).tolist() == POOLED
    tower = CLIPTextTower.from_text_model(model, dtype=dtype, device=DEV)
    padded = (mask == 0).to(DEV)
    h32 = {}
    for label, mk in (('no mask', None), ('right-padding mask', mask)):
        h32[label], e32 = reference(model, ids, mk)
        h16, e16 = reference(m16, ids, mk)
        out = tower(ids, attention_mask=mk)
        assert out[0] is out.last_hidden_state and out.last_hidden_state.dtype == dtype and out.pooler_output.dtype == dtype
        assert tuple(out.last_hidden_state.shape) == (3, 77, CONFIGS[name]['hidden']) and tuple(out.text_embeds.shape) == (3, 64)
        assert out.text_embeds.dtype == torch.float32
        assert torch.equal(tower.get_text_features(input_ids=ids, attention_mask=mk), out.text_embeds)
        for what, eh, r32, r16 in (('last_hidden_state', out.last_hidden_state.float(), h32[label], h16), ('text_embeds', out.text_embeds, e32, e16)):
            assert bool(torch.isfinite(eh).all())
            err_h, err_16, size = float((eh - r32).abs().max()), float((r16 - r32).abs().max()), float(r32.abs().max())
            print(f'CLIPTextTower {name} {DTN[dtype]} {label} {what}: max|e32| {size:.3e}, max|eh - e32| {err_h:.3e}, '
                  f'max|e16 - e32| {err_16:.3e}, ratio {err_h / err_16:.3f}')
            if what == 'last_hidden_state' and mk is not None:
                # the teeth of the mask comparison, from transformers alone: the mask moves the padded rows by far more than the yardstick
                moved = float(((h32['right-padding mask'] - h32['no mask']).abs() * padded[..., None]).max())
                print(f'    the mask moves the padded rows of e32 by {moved:.3e} (needs >= {30 * err_16:.3e})')
                assert moved >= 10 * 3 * err_16
                still = float(((h32['right-padding mask'] - h32['no mask']).abs() * (~padded)[..., None]).max())
                print(f'    and the valid rows by {still:.3e}')
            assert err_16 > 0 and err_h <= 3 * err_16


@pytest.mark.parametrize('name', ['w128', 'w128_legacy'])
def test_pooling_takes_the_end_token_rows(name):
    """rows 1 and 2 pool positions 8 and 39 under both eos rules (w128_legacy: the argmax branch)"""
    from diffusion_tts_amd import ops
    from diffusion_tts_amd.clip_text import CLIPTextTower
    model = text_model(name)
    tower = CLIPTextTower.from_text_model(model, dtype=torch.float16, device=DEV)
    assert tower.eos == CONFIGS[name]['eos']
    ids, mask = ids_and_mask(name)
    for mk in (None, mask):
        out = tower(ids, attention_mask=mk)
        want = out.last_hidden_state[torch.arange(3), torch.tensor(POOLED)]
        assert torch.equal(out.pooler_output, want)
        assert torch.equal(out.text_embeds, ops.linear(want.float().contiguous(), tower.w_proj))
        assert not torch.equal(out.pooler_output[1], out.last_hidden_state[1, 76])


# ---- the tower as the SD pipeline's text encoder ----------------------------------------------------------------------------------
def standins():
    """the U-Net and VAE decoder beside the text encoder, built as tests/test_gpu_sd_unet.py builds them (its `narrow` case); no search runs"""
    if 'standins' not in _MODELS:
        from diffusion_tts_amd import init as dinit
        from diffusion_tts_amd.sd_unet import SDUNet
        from diffusion_tts_amd.vae import VAEDecoder
        boc = (64, 128, 192, 192)
        unet = SDUNet(dinit.sd_unet_state_dict(boc, 2, 64, 2, seed=11), device=DEV, dtype=torch.float16, block_out_channels=boc,
                      attention_head_dim=2, cross_attention_dim=64, layers_per_block=2, sample_size=16)
        _MODELS['standins'] = unet, VAEDecoder(dinit.vae_decoder_state_dict(seed=5), device=DEV, dtype=torch.float16)
    return _MODELS['standins']


@pytest.mark.parametrize('dtype', DTYPES, ids=lambda d: DTN[d])
def test_pipeline_encodes_the_prompt_with_the_tower(dtype):
    from transformers import CLIPTextModel
    from diffusion_tts_amd.clip_text import CLIPTextTower
    from diffusion_tts_amd.sd_pipeline import SDSearchPipeline
    from sd_standins import TinyTokenizer
    unet, dec = standins()
    model = text_model('w128')
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        te32 = CLIPTextModel(text_config('w128')).eval().to(DEV)           # SD's text encoder class: [0] is last_hidden_state
    src = model.state_dict()                                               # (CLIPTextModel names its tensors with or without `text_model.`)
    te32.load_state_dict({k: src[k if k in src else 'text_model.' + k] for k in te32.state_dict()})
    te16 = copy.deepcopy(te32).to(dtype)
    tower = CLIPTextTower.from_text_model(model, dtype=dtype, device=DEV)
    tok = TinyTokenizer(vocab=1000)                                        # bos 998, end 999, padded to 77 with the end token
    enc = {}
    for label, te in (('e32', te32), ('e16', te16), ('eh', tower)):
        pipe = SDSearchPipeline(unet, dec, device=DEV, text_encoder=te, tokenizer=tok)
        enc[label] = pipe.encode_prompt('a prompt')
    for i, which in enumerate(('prompt', 'negative prompt')):
        eh, e32, e16 = enc['eh'][i], enc['e32'][i].float(), enc['e16'][i].float()
        assert eh.dtype == dtype and tuple(eh.shape) == (1, 77, 128) and e32.shape == eh.shape
        err_h, err_16 = float((eh.float() - e32).abs().max()), float((e16 - e32).abs().max())
        print(f'encode_prompt {DTN[dtype]} {which}: max|eh - e32| {err_h:.3e}, max|e16 - e32| {err_16:.3e}, ratio {err_h / err_16:.3f}')
        assert err_16 > 0 and err_h <= 3 * err_16
    assert not torch.equal(enc['eh'][0], enc['eh'][1])


# ---- the scorer ---------------------------------------------------------------------------------------------------------------------
PROMPT = ['a photo of a smooth field']


def clip_model():
    """a CLIPModel whose text side the kernels take (head dim 64): the `w128` text widths beside the `p32` vision tower of
    tests/test_gpu_clip_vision.py"""
    if 'clip' not in _MODELS:
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            from transformers import CLIPConfig, CLIPModel, CLIPVisionConfig
            vc = CLIPVisionConfig(hidden_size=128, intermediate_size=256, num_hidden_layers=2, num_attention_heads=2, image_size=224,
                                  patch_size=32, projection_dim=64)
            torch.manual_seed(1234)
            _MODELS['clip'] = CLIPModel(CLIPConfig(text_config=text_config('w128').to_dict(), vision_config=vc.to_dict(),
                                                   projection_dim=64)).eval().to(DEV)
    return _MODELS['clip']


def scorer_images(seed=11):
    """the eight 64x64 uint8 GPU images of tests/test_gpu_clip_vision.scorer_images, restated: smooth 7x7 random fields (bilinear) at 0.4
    contrast around a per-image colour level.  Kept for the text side after a check with transformers alone on the CPU, before the tower
    ran: for clip_model() and PROMPT the float32 rewards of these images spread over 0.378 where the reference's own 16-bit TEXT run
    errs by 2.7e-4 (float16) / 1.5e-3 (bfloat16) -- ratios 1400 / 255; the test needs 30 and re-measures both in place."""
    f = torch.rand(8, 3, 7, 7, generator=torch.Generator().manual_seed(seed))
    f = torch.nn.functional.interpolate(f, size=(64, 64), mode='bilinear', align_corners=False)
    tint = torch.rand(8, 3, 1, 1, generator=torch.Generator().manual_seed(3)) * 0.8 + 0.1
    return ((tint + (f - 0.5) * 0.4).clamp(0, 1) * 255).round().to(torch.uint8).to(DEV)


@pytest.mark.parametrize('dtype', DTYPES, ids=lambda d: DTN[d])
def test_scorer_with_the_text_tower(dtype):
    from diffusion_tts_amd import ops
    from diffusion_tts_amd.clip_text import CLIPTextTower
    from diffusion_tts_amd.scorers import CLIPScorer, _features
    model = clip_model()
    images = scorer_images()
    ref = CLIPScorer(model=model, device=DEV)
    hip = CLIPScorer(model=model, device=DEV, text_tower='hip', tower_dtype=dtype)
    assert isinstance(hip._text_tower, CLIPTextTower) and hip._text_tower.dtype == dtype and hip._tower is None and ref._text_tower is None
    seen = {}
    stock = model.get_image_features

    def record(pixel_values=None, **kw):
        out = stock(pixel_values=pixel_values, **kw)
        seen['img'] = _features(out).float().contiguous()
        return out

    model.get_image_features = record
    try:
        r32 = ref(images, PROMPT).float()
        img32 = seen['img']
        rh = hip(images, PROMPT).float()
    finally:
        del model.get_image_features
    assert torch.equal(seen['img'], img32) and hip._text_tower.rows == 8         # the same float32 image embedding on both sides
    # the reference's own 16-bit TEXT run: its text tower in the tower's type, the float32 image embedding, the same cosine tail
    enc = ref.tokenizer(PROMPT * 8, padding=True, truncation=True, max_length=77, return_tensors='pt').to(DEV)
    with torch.no_grad():
        t16 = _features(copy.deepcopy(model).to(dtype).get_text_features(**enc)).float().contiguous()
    r16 = ops.cosine_rows(img32, t16)
    err_h, err_16 = float((rh - r32).abs().max()), float((r16 - r32).abs().max())
    spread = float(r32.max() - r32.min())
    print(f'CLIPScorer text_tower=hip {DTN[dtype]}: fp32 reward spread {spread:.3e}, max|r_hip - r32| {err_h:.3e}, max|r16 - r32| {err_16:.3e}, '
          f'ratio {err_h / err_16:.3f}')
    assert err_16 > 0 and spread >= 10 * (3 * err_16)                             # else the comparison says nothing
    assert err_h <= 3 * err_16


# ---- the CLI ------------------------------------------------------------------------------------------------------------------------
def test_main_text_encoder_flag_reaches_the_loader(tmp_path):
    from conftest import ROOT
    sys.path.insert(0, ROOT)
    import main
    from diffusion_tts_amd.clip_text import CLIPTextTower
    base = ['--backend', 'sd', '--scorer', 'brightness']
    assert main.build_parser().parse_args(base).text_encoder == 'transformers'
    args = main.build_parser().parse_args(base + ['--text-encoder', 'hip'])
    model = text_model('w128')
    d = tmp_path / 'text_encoder'
    model.save_pretrained(str(d), safe_serialization=True)
    os.environ['DTS_SD_TEXT_ENCODER_DIR'] = str(d)
    try:
        te = main.load_sd_text_encoder('runwayml/stable-diffusion-v1-5', torch.device(DEV), args.text_encoder)
        os.environ['DTS_SD_TEXT_ENCODER_DIR'] = str(tmp_path / 'nothing')
        with pytest.raises(FileNotFoundError, match='DTS_SD_TEXT_ENCODER_DIR'):
            main.load_sd_text_encoder('runwayml/stable-diffusion-v1-5', torch.device(DEV), 'hip')
    finally:
        del os.environ['DTS_SD_TEXT_ENCODER_DIR']
    assert isinstance(te, CLIPTextTower) and te.dtype == torch.float16 and te.hidden == 128 and te.eos == 999
    assert not hasattr(te.config, 'use_attention_mask')
    ids, _ = ids_and_mask('w128')
    want = CLIPTextTower.from_text_model(model, dtype=torch.float16, device=DEV)(ids)
    got = te(ids)
    assert torch.equal(got[0], want[0]) and torch.equal(got.text_embeds, want.text_embeds)
    with pytest.raises(ValueError, match='--text-encoder'):
        main.load_sd_text_encoder('runwayml/stable-diffusion-v1-5', torch.device(DEV), 'triton')


# ---- determinism and refused input ------------------------------------------------------------------------------------------------
def test_forward_is_deterministic_rows_are_independent_and_bad_input_is_named():
    from diffusion_tts_amd.clip_text import CLIPTextTower
    tower = CLIPTextTower.from_text_model(text_model('w128'), dtype=torch.float16, device=DEV)
    ids, mask = ids_and_mask('w128')
    for mk in (None, mask):
        a, b = tower(ids, attention_mask=mk), tower(ids, attention_mask=mk)
        assert torch.equal(a[0], b[0]) and torch.equal(a.text_embeds, b.text_embeds)
        p = [0, 2, 1]
        c = tower(ids[p], attention_mask=None if mk is None else mk[p])
        for i, j in enumerate(p):
            assert torch.equal(c[0][i], a[0][j]) and torch.equal(c.text_embeds[i], a.text_embeds[j])
    assert torch.equal(tower(ids, attention_mask=torch.ones_like(mask))[0], tower(ids)[0])           # all ones: no mask
    with pytest.raises(ValueError, match='78 tokens exceed max_position_embeddings=77'):
        tower(torch.cat([ids, ids[:, :1]], 1))
    left = mask.flip(1)
    with pytest.raises(ValueError, match='row 1 is left-padded'):
        tower(ids, attention_mask=left)
    hole = mask.clone()
    hole[2, 5] = 0
    with pytest.raises(ValueError, match='row 2 has a hole'):
        tower(ids, attention_mask=hole)
    bad = ids.clone()
    bad[1, 3] = 1000
    with pytest.raises(ValueError, match='token id 1000 '):
        tower(bad)
