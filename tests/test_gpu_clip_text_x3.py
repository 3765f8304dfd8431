"""GPU: clip_text.CLIPTextTowerX3 (dtype ops.F16X3) and CLIPScorer(vision_tower='hip', text_tower='hip', tower_dtype='f16x3',
text_tower_dtype='f16x3') against transformers in float64.

The split-precision tower claims the float32 module's accuracy, so the yardstick is that of tests/test_gpu_clip_vision_x3.py: the float32
module's own distance from float64, measured in the same test on the same GPU -- x64 = the module's `.double()` copy, x32 = the module in
float32, x_hip = the tower; max|x_hip - x64| <= 4 max|x32 - x64| and err_32 > 0, for `last_hidden_state` (all tokens), `pooler_output` and
`text_embeds` separately.  Every ratio is printed.

Models (random init, torch.manual_seed(1234)); head dim 64 in both (the text settings of the other GPU tests have head dim 32, which this
tower refuses):
  t128   hidden 128, 2 heads, inter 256, 2 layers, vocab 1000, projection 64
  L      CLIP-L's text widths 768 / 12 / 3072, 2 layers, vocab 1000, projection 768
Inputs: three rows of 77 ids without a mask (row lengths 77 / 9 / 40: the pooled positions differ), and four rows of 77 ids with a
right-padding mask of lengths 3, 27, 65, 77 -- key lengths in the first tile, in the second tile and none.  The legacy eos_token_id == 2
pooling rule once (t128's widths).  Left padding and holes are refused by mask_key_len, as in the 16-bit tower.

The scorer test mirrors test_gpu_clip_vision_x3.test_scorer_at_the_float32_scorers_distance_from_float64 with BOTH towers on the kernels:
the p32 vision settings beside the t128 text settings, the eight 64x64 images of that file, eight prompts whose byte-tokenizer lengths are
27, 6, 65, 3 (t = 65: the longest prompt reaches into the second key tile); r64 has both towers in float64.
Measured on the MI355X (ratio max|x_hip - x64| / max|x32 - x64|, limit 4): t128 0.80 - 1.01 over the three outputs and both inputs (legacy
rule: the same figures), L 0.26 - 0.40; the scorer 0.97 (max|r32 - r64| 1.33e-7, smallest reward gap 4.4e-4: gap / (4 err_32) = 823).  Every
run prints its own figures."""
import copy
import warnings

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = 'cuda'
CONFIGS = {
    't128': dict(hidden=128, heads=2, inter=256, layers=2, vocab=1000, proj=64, eos=999),
    't128_legacy': dict(hidden=128, heads=2, inter=256, layers=2, vocab=1000, proj=64, eos=2),       # pooled at argmax(ids)
    'L': dict(hidden=768, heads=12, inter=3072, layers=2, vocab=1000, proj=768, eos=999),
}
BOS, END = 998, 999
PROMPTS = ['a photo of a smooth field', 'blue', 'a much longer prompt about nothing in particular at all, really', 'x'] * 2
_MODELS, _TOWERS = {}, {}


def text_config(name):
    from transformers import CLIPTextConfig
    c = CONFIGS[name]
    return CLIPTextConfig(vocab_size=c['vocab'], hidden_size=c['hidden'], intermediate_size=c['inter'], num_hidden_layers=c['layers'],
                          num_attention_heads=c['heads'], max_position_embeddings=77, projection_dim=c['proj'], bos_token_id=BOS,
                          eos_token_id=c['eos'], pad_token_id=END)


def text_model(name):
    if name not in _MODELS:
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            from transformers import CLIPTextModelWithProjection
            torch.manual_seed(1234)
            _MODELS[name] = CLIPTextModelWithProjection(text_config(name)).eval().to(DEV)
    return _MODELS[name]


def x3_tower(name):
    """one split-precision tower per model, shared by the tests (they only read it)"""
    if name not in _TOWERS:
        from diffusion_tts_amd.clip_text import CLIPTextTowerX3
        _TOWERS[name] = CLIPTextTowerX3.from_text_model(text_model(name), device=DEV)
    return _TOWERS[name]


def ids_and_mask(lens, seed=5):
    """len(lens) rows of 77 ids: bos, random ids, the end token at len - 1 and end-token padding after it; the right-padding mask"""
    ids = torch.randint(0, BOS, (len(lens), 77), generator=torch.Generator().manual_seed(seed))
    ids[:, 0] = BOS
    mask = torch.zeros(len(lens), 77, dtype=torch.long)
    for b, n in enumerate(lens):
        ids[b, n - 1:] = END
        mask[b, :n] = 1
    return ids, mask


def reference(model, ids, mask):
    """(last_hidden_state, pooler_output, text_embeds) of the transformers module, in its own precision"""
    with torch.no_grad():
        out = model.text_model(input_ids=ids.to(DEV), attention_mask=None if mask is None else mask.to(DEV))
        return out.last_hidden_state, out.pooler_output, model.text_projection(out.pooler_output)


def compare(label, tower, model, ids, mask):
    """the three outputs of the tower against the float64 module by the float32 module's own distance; returns the tower's output"""
    x32 = [x.double() for x in reference(model, ids, mask)]
    x64 = reference(copy.deepcopy(model).double(), ids, mask)
    assert all(x.dtype == torch.float64 for x in x64)
    out = tower(ids, attention_mask=mask)
    n, C = ids.shape[0], tower.hidden
    assert out[0] is out.last_hidden_state and tuple(out.last_hidden_state.shape) == (n, 77, C) and tuple(out.pooler_output.shape) == (n, C)
    assert tuple(out.text_embeds.shape) == (n, tower.proj_dim)
    bad = []
    for what, xh, r32, r64 in zip(('last_hidden_state', 'pooler_output', 'text_embeds'), (out.last_hidden_state, out.pooler_output, out.text_embeds),
                                  x32, x64):
        assert xh.dtype == torch.float32 and bool(torch.isfinite(xh).all()), what
        err_h, err_32, size = float((xh.double() - r64).abs().max()), float((r32 - r64).abs().max()), float(r64.abs().max())
        print(f'CLIPTextTowerX3 {label} {what}: max|x64| {size:.3e}, max|x_hip - x64| {err_h:.3e}, max|x32 - x64| {err_32:.3e}, '
              f'ratio {err_h / err_32 if err_32 > 0 else float("inf"):.3f}')
        assert err_32 > 0
        if not err_h <= 4 * err_32:
            bad.append((what, err_h, err_32))
    assert not bad, bad
    return out


@pytest.mark.parametrize('name', ['t128', 'L'])
def test_tower_at_the_float32_modules_distance_from_float64(name):
    from diffusion_tts_amd import ops
    from diffusion_tts_amd.clip_text import mask_key_len, pooled_positions
    model, tower = text_model(name), x3_tower(name)
    assert type(tower).__name__ == 'CLIPTextTowerX3' and tower.dtype == ops.F16X3 and tower.x3
    assert isinstance(tower.layers[0].w_qkv, ops.X3Weight) and isinstance(tower.layers[0].w_fc2, ops.X3Weight) and tower.w_proj.dtype == torch.float32
    ids, _ = ids_and_mask((77, 9, 40))
    assert pooled_positions(ids, CONFIGS[name]['eos']).tolist() == [76, 8, 39]
    out = compare(f'{name} no mask', tower, model, ids, None)
    assert torch.equal(out.pooler_output, out.last_hidden_state[torch.arange(3), torch.tensor([76, 8, 39])])
    assert torch.equal(tower.get_text_features(input_ids=ids), out.text_embeds)
    ids, mask = ids_and_mask((3, 27, 65, 77), seed=6)
    assert mask_key_len(mask, 4, 77).tolist() == [3, 27, 65, 77]
    masked = compare(f'{name} right-padding mask', tower, model, ids, mask)
    # the mask reaches the kernel: the padded rows of the masked run differ from the unmasked run's, the rows in front of them do not
    plain = tower(ids)
    assert torch.equal(masked.last_hidden_state[0, :3], plain.last_hidden_state[0, :3])
    assert not torch.equal(masked.last_hidden_state[0, 3:], plain.last_hidden_state[0, 3:])
    assert torch.equal(masked.last_hidden_state[3], plain.last_hidden_state[3])


def test_the_legacy_eos_rule_pools_at_the_largest_id():
    from diffusion_tts_amd.clip_text import pooled_positions
    model, tower = text_model('t128_legacy'), x3_tower('t128_legacy')
    assert tower.eos == 2
    ids, _ = ids_and_mask((77, 9, 40))
    assert pooled_positions(ids, 2).tolist() == [76, 8, 39]
    out = compare('t128_legacy no mask', tower, model, ids, None)
    assert torch.equal(out.pooler_output, out.last_hidden_state[torch.arange(3), torch.tensor([76, 8, 39])])
    assert not torch.equal(out.pooler_output[1], out.last_hidden_state[1, 76])


def test_forward_is_deterministic_rows_are_independent_and_bad_input_is_named():
    tower = x3_tower('t128')
    ids, mask = ids_and_mask((3, 27, 65, 77), seed=6)
    for mk in (None, mask):
        a, b = tower(ids, attention_mask=mk), tower(ids, attention_mask=mk)
        assert torch.equal(a[0], b[0]) and torch.equal(a.text_embeds, b.text_embeds)
        p = [2, 0, 3, 1]
        c = tower(ids[p], attention_mask=None if mk is None else mk[p])
        for i, j in enumerate(p):
            assert torch.equal(c[0][i], a[0][j]) and torch.equal(c.text_embeds[i], a.text_embeds[j])
    assert torch.equal(tower(ids, attention_mask=torch.ones_like(mask))[0], tower(ids)[0])           # all ones: no mask
    short = tower(ids[:, :1])                                                                         # t = 1: a single key
    assert tuple(short[0].shape) == (4, 1, 128) and bool(torch.isfinite(short[0]).all())
    with pytest.raises(ValueError, match='78 tokens exceed max_position_embeddings=77'):
        tower(torch.cat([ids, ids[:, :1]], 1))
    with pytest.raises(ValueError, match='row 0 is left-padded'):
        tower(ids, attention_mask=mask.flip(1))
    hole = mask.clone()
    hole[2, 5] = 0
    with pytest.raises(ValueError, match='row 2 has a hole'):
        tower(ids, attention_mask=hole)
    bad = ids.clone()
    bad[1, 3] = 1000
    with pytest.raises(ValueError, match='token id 1000 '):
        tower(bad)


@pytest.mark.parametrize('c', [64, 768])
@pytest.mark.parametrize('t', [1, 77])
def test_text_tokens_f32_is_one_float32_add(t, c):
    from diffusion_tts_amd import ops
    vocab, n = 1000, 3
    g = torch.Generator().manual_seed(100 * t + c)
    tok, pos = torch.randn(vocab, c, generator=g), torch.randn(77, c, generator=g)
    ids = torch.randint(0, vocab, (n, t), generator=g)
    ids[0, 0], ids[1, 0], ids[2, 0] = 0, vocab - 1, vocab - 1           # the two ends of the table, and a repeat
    got = ops.text_tokens_f32(ids, tok.to(DEV), pos.to(DEV))
    assert got.dtype == torch.float32 and tuple(got.shape) == (n, t, c) and torch.equal(got.cpu(), tok[ids] + pos[:t])
    assert torch.equal(ops.text_tokens_f32(ids.to(DEV).to(torch.int32), tok.to(DEV), pos.to(DEV)), got)
    wrong = ids.clone()
    wrong[n - 1, t - 1] = vocab
    with pytest.raises(ValueError, match=f'text_tokens_f32: token id {vocab} '):
        ops.text_tokens_f32(wrong, tok.to(DEV), pos.to(DEV))


# ---- the scorer ---------------------------------------------------------------------------------------------------------------------
def clip_model():
    """the `p32` vision settings of tests/test_gpu_clip_vision_x3.py beside the `t128` text settings"""
    if 'clip' not in _MODELS:
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            from transformers import CLIPConfig, CLIPModel, CLIPVisionConfig
            vc = CLIPVisionConfig(hidden_size=128, intermediate_size=256, num_hidden_layers=2, num_attention_heads=2, image_size=224,
                                  patch_size=32, projection_dim=64)
            torch.manual_seed(1234)
            _MODELS['clip'] = CLIPModel(CLIPConfig(text_config=text_config('t128').to_dict(), vision_config=vc.to_dict(),
                                                   projection_dim=64)).eval().to(DEV)
    return _MODELS['clip']


def scorer_images(seed=11):
    """the eight 64x64 uint8 GPU images of tests/test_gpu_clip_vision_x3.py"""
    f = torch.rand(8, 3, 7, 7, generator=torch.Generator().manual_seed(seed))
    f = torch.nn.functional.interpolate(f, size=(64, 64), mode='bilinear', align_corners=False)
    tint = torch.rand(8, 3, 1, 1, generator=torch.Generator().manual_seed(3)) * 0.8 + 0.1
    return ((tint + (f - 0.5) * 0.4).clamp(0, 1) * 255).round().to(torch.uint8).to(DEV)


def test_scorer_with_both_towers_at_the_float32_scorers_distance_from_float64():
    from diffusion_tts_amd import ops
    from diffusion_tts_amd.scorers import CLIPScorer, _features
    model = clip_model()
    images = scorer_images()
    ref = CLIPScorer(model=model, device=DEV)
    enc = ref.tokenizer(PROMPTS, padding=True, truncation=True, max_length=77, return_tensors='pt')
    assert tuple(enc['input_ids'].shape) == (8, 65) and enc['attention_mask'].sum(-1).tolist() == [27, 6, 65, 3] * 2
    seen = {}
    stock = model.get_image_features

    def record_ref(pixel_values=None, **kw):
        seen['ref'] = pixel_values.clone()
        return stock(pixel_values=pixel_values, **kw)

    model.get_image_features = record_ref
    try:
        r32 = ref(images, PROMPTS).double()
    finally:
        del model.get_image_features
    assert ref.device_preprocessed == 8 and seen['ref'].dtype == torch.float32
    # r64: BOTH towers in float64 on the same pixel_values and the same ids, the cosine in float64
    m64 = copy.deepcopy(model).double()
    with torch.no_grad():
        e64 = _features(m64.get_image_features(pixel_values=seen['ref'].double()))
        t64 = _features(m64.get_text_features(**enc.to(DEV)))
    assert e64.dtype == torch.float64 and t64.dtype == torch.float64
    r64 = (torch.nn.functional.normalize(e64, dim=-1) * torch.nn.functional.normalize(t64, dim=-1)).sum(-1)
    err_32 = float((r32 - r64).abs().max())
    order32 = torch.argsort(r32)
    gap, spread = float(r32[order32].diff().min()), float(r32.max() - r32.min())
    print(f'CLIPScorer p32 + t128, eight prompts: fp32 reward spread {spread:.3e}, smallest gap {gap:.3e}, max|r32 - r64| {err_32:.3e}, '
          f'gap / (4 err_32) {gap / (4 * err_32) if err_32 > 0 else float("inf"):.0f}')
    # from transformers alone, before the towers run: the ranking is decided far above the allowed error, else the comparison says nothing
    assert err_32 > 0 and gap >= 100 * (4 * err_32)
    assert torch.equal(order32, torch.argsort(r64))
    hip = CLIPScorer(model=model, device=DEV, vision_tower='hip', text_tower='hip', tower_dtype=ops.F16X3, text_tower_dtype=ops.F16X3)
    assert type(hip._tower).__name__ == 'CLIPVisionTowerX3' and type(hip._text_tower).__name__ == 'CLIPTextTowerX3'
    assert hip._text_tower.dtype == ops.F16X3
    rh = hip(images, PROMPTS).double()
    assert hip.device_preprocessed == 8 and hip._tower.rows == 8 and hip._text_tower.rows == 8
    err_h = float((rh - r64).abs().max())
    print(f'CLIPScorer both towers f16x3: max|r_hip - r64| {err_h:.3e}, max|r32 - r64| {err_32:.3e}, ratio {err_h / err_32:.3f}')
    assert err_h <= 4 * err_32
    assert torch.equal(torch.argsort(rh), order32)
    again = hip(images, PROMPTS).double()                                 # the same prompts: the text cache answers, the tower does not run
    assert hip._text_tower.rows == 8 and hip._tower.rows == 16 and torch.equal(again, rh)


def test_text_tower_dtype_selects_the_text_towers_class_whatever_the_image_towers_is():
    from diffusion_tts_amd import ops
    from diffusion_tts_amd.scorers import CLIPScorer
    model = clip_model()
    s = CLIPScorer(model=model, device=DEV, vision_tower='hip', text_tower='hip', tower_dtype=ops.F16X3, text_tower_dtype=torch.float16)
    assert type(s._tower).__name__ == 'CLIPVisionTowerX3' and type(s._text_tower).__name__ == 'CLIPTextTower' and s._text_tower.dtype == torch.float16
    s = CLIPScorer(model=model, device=DEV, text_tower='hip', text_tower_dtype=ops.F16X3)
    assert s._tower is None and type(s._text_tower).__name__ == 'CLIPTextTowerX3'
    s = CLIPScorer(model=model, device=DEV, text_tower='hip', tower_dtype=torch.bfloat16)             # None: borrows tower_dtype, as before
    assert type(s._text_tower).__name__ == 'CLIPTextTower' and s._text_tower.dtype == torch.bfloat16
    r = CLIPScorer(model=model, device=DEV, text_tower='hip', text_tower_dtype=ops.F16X3)(scorer_images(), PROMPTS[:1])
    assert tuple(r.shape) == (8,) and bool(torch.isfinite(r).all())


def test_main_clip_text_tower_flags_reach_the_tower():
    import main
    from diffusion_tts_amd import ops
    args = main.build_parser().parse_args(['--backend', 'sd', '--scorer', 'clip', '--clip-tower', 'hip', '--clip-tower-dtype', 'f16x3',
                                           '--clip-text-tower', 'hip', '--clip-text-tower-dtype', 'f16x3'])
    scorer = main.get_scorer('sd', 'clip', torch.device(DEV), clip_tower=args.clip_tower, clip_model=clip_model(),
                             clip_tower_dtype=args.clip_tower_dtype, clip_text_tower=args.clip_text_tower,
                             clip_text_tower_dtype=args.clip_text_tower_dtype)
    assert scorer.text_tower == 'hip' and type(scorer._text_tower).__name__ == 'CLIPTextTowerX3' and scorer._tower.dtype == ops.F16X3
    r = scorer(scorer_images(), PROMPTS)
    assert tuple(r.shape) == (8,) and bool(torch.isfinite(r).all()) and scorer._text_tower.rows == 8
