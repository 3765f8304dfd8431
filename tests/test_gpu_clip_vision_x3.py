"""GPU: clip_vision.CLIPVisionTowerX3 (dtype ops.F16X3) and CLIPScorer(vision_tower='hip', tower_dtype=ops.F16X3) against transformers in float64.

The split-precision tower claims the float32 module's accuracy, so the yardstick is the float32 module's own distance from float64, measured in
the same test on the same GPU: e64 = get_image_features of the module in float64, e32 = the module in float32, eh = the tower;
max|eh - e64| <= 4 max|e32 - e64| -- the margin this project uses for parity-grade modes against the reference's own f32-vs-f64 distance
(tests/test_gpu_ncsnpp.py).  The models, inputs and scorer images are those of tests/test_gpu_clip_vision.py (random init, fixed seed; smooth
fields; three rows, an odd count on purpose); its small helpers are repeated here.  L14x2 has 257 tokens at head dim 64, so it takes
dts_attention_x3 and the fused operand images; p14 and p32 (17 / 50 tokens) take the float32 attention.
"""
import copy
import warnings

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = 'cuda'
MEAN = torch.tensor([0.48145466, 0.4578275, 0.40821073]).view(1, 3, 1, 1)
STD = torch.tensor([0.26862954, 0.26130258, 0.27577711]).view(1, 3, 1, 1)
CONFIGS = {
    'p14': dict(hidden=128, heads=2, inter=256, layers=2, image=56, patch=14, proj=64),          # T = 17
    'p32': dict(hidden=128, heads=2, inter=256, layers=2, image=224, patch=32, proj=64),         # T = 50
    'L14x2': dict(hidden=1024, heads=16, inter=4096, layers=2, image=224, patch=14, proj=768),   # ViT-L/14's widths, T = 257
}
_MODELS, _TOWERS = {}, {}


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


def x3_tower(name):
    """one split-precision tower per model, shared by the tests (they only read it)"""
    if name not in _TOWERS:
        from diffusion_tts_amd.clip_vision import CLIPVisionTowerX3
        _TOWERS[name] = CLIPVisionTowerX3.from_clip_model(clip_model(name), device=DEV)
    return _TOWERS[name]


def fields(n, size, seed):
    """n smooth images in [0, 1], [n, 3, size, size]: a 7x7 random field interpolated to the image size"""
    f = torch.rand(n, 3, 7, 7, generator=torch.Generator().manual_seed(seed))
    return torch.nn.functional.interpolate(f, size=(size, size), mode='bicubic', align_corners=False).clamp(0, 1)


def scorer_images(seed=11):
    """the eight 64x64 uint8 GPU images of tests/test_gpu_clip_vision.py"""
    f = torch.rand(8, 3, 7, 7, generator=torch.Generator().manual_seed(seed))
    f = torch.nn.functional.interpolate(f, size=(64, 64), mode='bilinear', align_corners=False)
    tint = torch.rand(8, 3, 1, 1, generator=torch.Generator().manual_seed(3)) * 0.8 + 0.1
    return ((tint + (f - 0.5) * 0.4).clamp(0, 1) * 255).round().to(torch.uint8).to(DEV)


def pixel_values(n, size, seed):
    return ((fields(n, size, seed) - MEAN) / STD).to(DEV).contiguous()


def feats(model, pix):
    out = model.get_image_features(pixel_values=pix)
    return out if isinstance(out, torch.Tensor) else out.pooler_output


@pytest.mark.parametrize('name', list(CONFIGS))
def test_tower_at_the_float32_modules_distance_from_float64(name):
    from diffusion_tts_amd import ops
    model = clip_model(name)
    pix = pixel_values(3, CONFIGS[name]['image'], 7)
    with torch.no_grad():
        e32 = feats(model, pix).double()
        e64 = feats(copy.deepcopy(model).double(), pix.double())
    assert e64.dtype == torch.float64
    tower = x3_tower(name)
    assert tower.dtype == ops.F16X3 and isinstance(tower.layers[0].w_qkv, ops.X3Weight) and isinstance(tower.w_patch, ops.X3Weight)
    assert ops.attention_x3_ok(tower.tokens, tower.hidden // tower.heads) == (name == 'L14x2')
    eh = tower(pix)
    assert eh.dtype == torch.float32 and tuple(eh.shape) == (3, CONFIGS[name]['proj']) and bool(torch.isfinite(eh).all())
    err_h, err_32, size = float((eh.double() - e64).abs().max()), float((e32 - e64).abs().max()), float(e64.abs().max())
    print(f'CLIPVisionTowerX3 {name} f16x3: max|e64| {size:.3e}, max|eh - e64| {err_h:.3e}, max|e32 - e64| {err_32:.3e}, ratio {err_h / err_32:.3f}')
    assert err_32 > 0
    assert err_h <= 4 * err_32


def test_scorer_at_the_float32_scorers_distance_from_float64():
    from diffusion_tts_amd import ops
    from diffusion_tts_amd.scorers import CLIPScorer
    model = clip_model('p32')
    images = scorer_images()
    prompt = ['a photo of a smooth field']
    ref = CLIPScorer(model=model, device=DEV)
    seen = {}
    stock = model.get_image_features

    def record_ref(pixel_values=None, **kw):
        seen['ref'] = pixel_values.clone()
        return stock(pixel_values=pixel_values, **kw)

    model.get_image_features = record_ref
    try:
        r32 = ref(images, prompt).double()
    finally:
        del model.get_image_features
    assert ref.device_preprocessed == 8 and seen['ref'].dtype == torch.float32
    # r64: the float64 image tower on the same pixel_values, the same float32 text embedding, the cosine in float64
    txt = next(iter(ref._text_cache.values())).double()
    with torch.no_grad():
        e64 = feats(copy.deepcopy(model).double(), seen['ref'].double())
    r64 = (torch.nn.functional.normalize(e64, dim=-1) * torch.nn.functional.normalize(txt, dim=-1)).sum(-1)
    err_32 = float((r32 - r64).abs().max())
    order32 = torch.argsort(r32)
    gap, spread = float(r32[order32].diff().min()), float(r32.max() - r32.min())
    print(f'CLIPScorer p32: fp32 reward spread {spread:.3e}, smallest gap {gap:.3e}, max|r32 - r64| {err_32:.3e}')
    # from transformers alone, before the tower runs: the ranking is decided far above the allowed error, else the comparison says nothing
    assert err_32 > 0 and gap >= 100 * (4 * err_32)
    assert torch.equal(order32, torch.argsort(r64))
    hip = CLIPScorer(model=model, device=DEV, vision_tower='hip', tower_dtype=ops.F16X3)
    tower = hip._tower
    assert type(tower).__name__ == 'CLIPVisionTowerX3' and tower.dtype == ops.F16X3 and hip._text_tower is None

    def record_hip(pix):
        seen['hip'] = pix.clone()
        return tower(pix)

    hip._tower = record_hip
    try:
        rh = hip(images, prompt).double()
    finally:
        hip._tower = tower
    assert hip.device_preprocessed == 8 and tower.rows == 8
    assert torch.equal(seen['ref'], seen['hip'])                                                   # both towers see the same pixel_values
    err_h = float((rh - r64).abs().max())
    print(f'CLIPScorer p32 f16x3: max|r_hip - r64| {err_h:.3e}, max|r32 - r64| {err_32:.3e}, ratio {err_h / err_32:.3f}')
    assert err_h <= 4 * err_32
    assert torch.equal(torch.argsort(rh), order32)


@pytest.mark.parametrize('name', ['p14', 'L14x2'])
def test_forward_is_deterministic_and_rows_are_independent(name):
    tower = x3_tower(name)
    pix = pixel_values(3, CONFIGS[name]['image'], 21)
    a = tower(pix)
    assert torch.equal(a, tower(pix))
    b = tower(pix[[0, 2, 1]].contiguous())
    assert torch.equal(b[0], a[0]) and torch.equal(b[1], a[2]) and torch.equal(b[2], a[1])
    with pytest.raises(ValueError, match='pixel_values'):
        tower(pix[:, :2].contiguous())


def test_forward_makes_no_host_synchronisation():
    tower = x3_tower('p14')
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


def test_the_float16_tower_is_the_same_launches_as_before():
    """the 16-bit forward did not change with the new mode: the float16 tower's output on p14 equals, bit for bit, the launch sequence of the
    16-bit tower written out by hand from ops (patchify, 1x1 conv, vit_tokens, layer_norm, per layer layer_norm - qkv conv - attention -
    out_proj conv with residual - layer_norm - fc1 conv - in-place gelu - fc2 conv with residual, vit_head, linear)"""
    from diffusion_tts_amd import ops
    from diffusion_tts_amd.clip_vision import CLIPVisionTower
    t = CLIPVisionTower.from_clip_model(clip_model('p14'), dtype=torch.float16, device=DEV)
    assert not t.x3 and t.layers[0].w_qkv.dtype == torch.float16
    pix = pixel_values(3, 56, 7)
    n, C, T, g = 3, t.hidden, t.tokens, t.grid
    rows = ops.patchify(pix, t.patch, torch.float16, t.kpad)
    emb = ops.conv2d(rows.view(n, g, g, t.kpad), t.w_patch)
    h = ops.vit_tokens(emb.view(n, g * g, C), t.cls, t.pos)
    h = ops.layer_norm(h, *t.pre_ln, eps=t.eps).view(n, T, 1, C)
    for P in t.layers:
        y = ops.layer_norm(h, *P.ln1, eps=t.eps)
        qkv = ops.conv2d(y, P.w_qkv, P.b_qkv)
        a = ops.attention(qkv.view(n, T, 3 * C), t.heads, t.scale)
        h = ops.conv2d(a.view(n, T, 1, C), P.w_o, P.b_o, residual=h)
        y = ops.layer_norm(h, *P.ln2, eps=t.eps)
        f = ops.conv2d(y, P.w_fc1, P.b_fc1)
        ops.gelu(f, t.act, out=f)
        h = ops.conv2d(f, P.w_fc2, P.b_fc2, residual=h)
    want = ops.linear(ops.vit_head(h.view(n, T, C), *t.post_ln, eps=t.eps), t.w_proj)
    got = t(pix)
    assert got.dtype == torch.float32 and torch.equal(got, want)
    # and the calls it makes are exactly those: none of the split-precision ops
    calls = []
    names = ['patchify', 'conv2d', 'vit_tokens', 'layer_norm', 'attention', 'gelu', 'vit_head', 'linear', 'layer_norm_x3', 'gelu_x3',
             'patchify_x3', 'vit_tokens_f32', 'vit_head_f32', 'split3_f16']
    saved = {k: getattr(ops, k) for k in names}
    try:
        for k in names:
            setattr(ops, k, (lambda k_: lambda *a_, **kw_: (calls.append(k_), saved[k_](*a_, **kw_))[1])(k))
        assert torch.equal(t(pix), want)
    finally:
        for k in names:
            setattr(ops, k, saved[k])
    per_layer = ['layer_norm', 'conv2d', 'attention', 'conv2d', 'layer_norm', 'conv2d', 'gelu', 'conv2d']
    assert calls == ['patchify', 'conv2d', 'vit_tokens', 'layer_norm'] + per_layer * len(t.layers) + ['vit_head', 'linear']


def test_main_clip_tower_dtype_flag_reaches_the_tower():
    import main
    from diffusion_tts_amd import ops
    args = main.build_parser().parse_args(['--backend', 'sd', '--scorer', 'clip', '--clip-tower', 'hip', '--clip-tower-dtype', 'f16x3'])
    scorer = main.get_scorer('sd', 'clip', torch.device(DEV), clip_tower=args.clip_tower, clip_model=clip_model('p32'),
                             clip_tower_dtype=args.clip_tower_dtype)
    assert scorer.vision_tower == 'hip' and scorer._tower.dtype == ops.F16X3 and scorer._tower.x3
    r = scorer(scorer_images(), ['a photo of a smooth field'])
    assert tuple(r.shape) == (8,) and bool(torch.isfinite(r).all()) and scorer._tower.rows == 8
