"""GPU: clip_vision.CLIPVisionTower and CLIPScorer(vision_tower='hip') against transformers itself -- the module the reference calls.

The tower computes in float16 / bfloat16 where the reference scores in float32, so the yardstick is the REFERENCE'S OWN 16-bit error,
measured in the same test: e32 = get_image_features in float32, e16 = the same module and input cast to the tower's type, eh = the HIP
tower; max|eh - e32| <= 3 max|e16 - e32| (the margin this project uses for 16-bit modules against the reference, tests/test_gpu_sd_unet.py).
Random-init models with a fixed seed; inputs are smooth fields (a 7x7 random field interpolated to the image size, then normalised), three
rows -- an odd count on purpose."""
import copy
import warnings

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = 'cuda'
DTYPES = [torch.float16, torch.bfloat16]
MEAN = torch.tensor([0.48145466, 0.4578275, 0.40821073]).view(1, 3, 1, 1)
STD = torch.tensor([0.26862954, 0.26130258, 0.27577711]).view(1, 3, 1, 1)
CONFIGS = {
    'p14': dict(hidden=128, heads=2, inter=256, layers=2, image=56, patch=14, proj=64),          # T = 17
    'p32': dict(hidden=128, heads=2, inter=256, layers=2, image=224, patch=32, proj=64),         # T = 50
    'L14x2': dict(hidden=1024, heads=16, inter=4096, layers=2, image=224, patch=14, proj=768),   # ViT-L/14's widths, T = 257
}
_MODELS = {}


def clip_model(name):
    if name not in _MODELS:
        c = CONFIGS[name]
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            from transformers import CLIPConfig, CLIPModel, CLIPTextConfig, CLIPVisionConfig
            tc = CLIPTextConfig(vocab_size=1000, hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=2,
                                max_position_embeddings=77, projection_dim=c['proj'], bos_token_id=998, eos_token_id=999, pad_token_id=999)
            vc = CLIPVisionConfig(hidden_size=c['hidden'], intermediate_size=c['inter'], num_hidden_layers=c['layers'],
                                  num_attention_heads=c['heads'], image_size=c['image'], patch_size=c['patch'], projection_dim=c['proj'])
            torch.manual_seed(1234)
            _MODELS[name] = CLIPModel(CLIPConfig(text_config=tc.to_dict(), vision_config=vc.to_dict(), projection_dim=c['proj'])).eval().to(DEV)
    return _MODELS[name]


def fields(n, size, seed):
    """n smooth images in [0, 1], [n, 3, size, size]: a 7x7 random field interpolated to the image size"""
    f = torch.rand(n, 3, 7, 7, generator=torch.Generator().manual_seed(seed))
    return torch.nn.functional.interpolate(f, size=(size, size), mode='bicubic', align_corners=False).clamp(0, 1)


def scorer_images(seed=11):
    """eight 64x64 uint8 GPU images for the scorer: such fields (bilinear) at 0.4 contrast around a per-image colour level, as the candidates
    of a search differ in colour and brightness.  Chosen with transformers alone on the CPU, before the tower ran: for the p32 model the
    float32 rewards of these images spread over 0.043 where the reference's own bfloat16 run errs by 8.0e-4 (ratio 54; the test needs 30)."""
    f = torch.rand(8, 3, 7, 7, generator=torch.Generator().manual_seed(seed))
    f = torch.nn.functional.interpolate(f, size=(64, 64), mode='bilinear', align_corners=False)
    tint = torch.rand(8, 3, 1, 1, generator=torch.Generator().manual_seed(3)) * 0.8 + 0.1
    return ((tint + (f - 0.5) * 0.4).clamp(0, 1) * 255).round().to(torch.uint8).to(DEV)


def pixel_values(n, size, seed):
    return ((fields(n, size, seed) - MEAN) / STD).to(DEV).contiguous()


def feats(model, pix):
    out = model.get_image_features(pixel_values=pix)
    return (out if isinstance(out, torch.Tensor) else out.pooler_output).float()


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('name', list(CONFIGS))
def test_tower_against_transformers(name, dtype):
    from diffusion_tts_amd.clip_vision import CLIPVisionTower
    model = clip_model(name)
    pix = pixel_values(3, CONFIGS[name]['image'], 7)
    with torch.no_grad():
        e32 = feats(model, pix)
        e16 = feats(copy.deepcopy(model).to(dtype), pix.to(dtype))
    tower = CLIPVisionTower.from_clip_model(model, dtype=dtype, device=DEV)
    assert tower.tokens == (CONFIGS[name]['image'] // CONFIGS[name]['patch']) ** 2 + 1
    eh = tower(pix)
    assert eh.dtype == torch.float32 and tuple(eh.shape) == (3, CONFIGS[name]['proj']) and bool(torch.isfinite(eh).all())
    err_h, err_16, size = float((eh - e32).abs().max()), float((e16 - e32).abs().max()), float(e32.abs().max())
    print(f'CLIPVisionTower {name} {str(dtype).split(".")[-1]}: max|e32| {size:.3e}, max|eh - e32| {err_h:.3e}, max|e16 - e32| {err_16:.3e}, '
          f'ratio {err_h / err_16:.3f}')
    assert err_16 > 0 and err_h <= 3 * err_16


@pytest.mark.parametrize('dtype', DTYPES)
def test_scorer_against_transformers(dtype):
    from diffusion_tts_amd import ops
    from diffusion_tts_amd.scorers import CLIPScorer
    model = clip_model('p32')
    images = scorer_images()
    prompt = ['a photo of a smooth field']
    ref = CLIPScorer(model=model, device=DEV)
    hip = CLIPScorer(model=model, device=DEV, vision_tower='hip', tower_dtype=dtype)
    seen = {}
    stock, tower = model.get_image_features, hip._tower

    def record_ref(pixel_values=None, **kw):
        seen['ref'] = pixel_values.clone()
        return stock(pixel_values=pixel_values, **kw)

    def record_hip(pix):
        seen['hip'] = pix.clone()
        return tower(pix)

    model.get_image_features, hip._tower = record_ref, record_hip
    try:
        r32 = ref(images, prompt).float()
        rh = hip(images, prompt).float()
    finally:
        del model.get_image_features
        hip._tower = tower
    assert ref.device_preprocessed == 8 and hip.device_preprocessed == 8 and tower.rows == 8
    assert seen['ref'].dtype == torch.float32 and torch.equal(seen['ref'], seen['hip'])           # both towers see the same pixel_values
    # the reference's own 16-bit run: its image tower and input in the tower's type, the same float32 text embedding
    with torch.no_grad():
        e16 = feats(copy.deepcopy(model).to(dtype), seen['ref'].to(dtype)).contiguous()
    txt = next(iter(ref._text_cache.values()))
    r16 = ops.cosine_rows(e16, txt)
    err_h, err_16 = float((rh - r32).abs().max()), float((r16 - r32).abs().max())
    spread = float(r32.max() - r32.min())
    print(f'CLIPScorer p32 {str(dtype).split(".")[-1]}: fp32 reward spread {spread:.3e}, max|r_hip - r32| {err_h:.3e}, max|r16 - r32| {err_16:.3e}, '
          f'ratio {err_h / err_16:.3f}')
    assert err_16 > 0 and spread >= 10 * (3 * err_16)                                              # else the comparison says nothing
    assert err_h <= 3 * err_16


def test_forward_is_deterministic_and_rows_are_independent():
    from diffusion_tts_amd.clip_vision import CLIPVisionTower
    tower = CLIPVisionTower.from_clip_model(clip_model('p14'), dtype=torch.float16, device=DEV)
    pix = pixel_values(3, 56, 21)
    a = tower(pix)
    assert torch.equal(a, tower(pix))
    b = tower(pix[[0, 2, 1]].contiguous())
    assert torch.equal(b[0], a[0]) and torch.equal(b[1], a[2]) and torch.equal(b[2], a[1])
    with pytest.raises(ValueError, match='pixel_values'):
        tower(pixel_values(1, 42, 0))
    with pytest.raises(ValueError, match='pixel_values'):
        tower(pix[:, :2].contiguous())


def test_forward_makes_no_host_synchronisation():
    from diffusion_tts_amd.clip_vision import CLIPVisionTower
    tower = CLIPVisionTower.from_clip_model(clip_model('p14'), dtype=torch.float16, device=DEV)
    pix = pixel_values(3, 56, 22)
    warm = tower(pix)
    torch.cuda.synchronize()
    before = torch.cuda.get_sync_debug_mode()
    try:
        torch.cuda.set_sync_debug_mode('error')
        out = tower(pix)
    finally:
        torch.cuda.set_sync_debug_mode(before)
    assert torch.equal(out, warm)


def test_main_clip_tower_flag_reaches_the_tower():
    import main
    from diffusion_tts_amd.clip_vision import CLIPVisionTower
    args = main.build_parser().parse_args(['--backend', 'sd', '--scorer', 'clip', '--clip-tower', 'hip'])
    model = clip_model('p32')
    scorer = main.get_scorer('sd', 'clip', torch.device(DEV), clip_tower=args.clip_tower, clip_model=model)
    assert isinstance(scorer._tower, CLIPVisionTower) and scorer.vision_tower == 'hip' and scorer._tower.dtype == torch.float16
    images = scorer_images()
    r = scorer(images, ['a photo of a smooth field'])
    assert tuple(r.shape) == (8,) and bool(torch.isfinite(r).all()) and scorer._tower.rows == 8
    stock = main.get_scorer('sd', 'clip', torch.device(DEV), clip_model=model)
    assert stock._tower is None and stock.vision_tower == 'transformers'
