"""Pins tests/conv_reference.py on the CPU.  conv_ref64 against torch's float64 conv2d (the one place F.conv2d is allowed near it); the
exactness conditions of every launch of the table (so the GPU file's equalities are fair: the reference alone stays inside them); and the
teeth of the net -- each indexing mistake a kernel could make, applied to the REFERENCE, changes at least one output element of every case
it applies to, so the sparse integer inputs do not hide such faults (the counts are printed)."""
import pytest
import torch
import torch.nn.functional as F

import conv_reference as R
from conv_reference import ABSENT, CASES, FORMS, MODES, STORE

CASE_MODE = sorted({(c, m) for c, m, _ in R.launches()})


def _args_ref(name, mode, variant='int'):
    a = R.exact_inputs(name, mode, 0, variant)
    return a, R.reference(a)


def _out_dtype(case, mode):
    return torch.float32 if case.form.startswith('out3') else STORE[mode]


@pytest.mark.parametrize('name', list(CASES))
def test_conv_ref64_is_float64_conv2d(name):
    case = CASES[name]
    for variant in case.variants:
        mode = case.modes[-1] if variant != 'int' else case.modes[0]
        a, ref = _args_ref(name, mode, variant)
        x = a['x1'] if a['x2'] is None else torch.cat([a['x1'], a['x2']], 1)
        if a['gn'] is not None:
            x = x * a['gn'][0][:, :, None, None] + a['gn'][1][:, :, None, None]
        if case.up:
            x = F.interpolate(x, scale_factor=2, mode='nearest')
        want = F.conv2d(x, a['w'], a['bias'], padding=case.k // 2)
        if a['skip'] is not None:
            src, ws, s_up = a['skip']
            want = want + F.conv2d(F.interpolate(src, scale_factor=2, mode='nearest') if s_up else src, ws)
        if a['bias_nc'] is not None:
            want = want + a['bias_nc'][:, :, None, None]
        if a['residual'] is not None:
            want = want + a['residual']
        want = want * case.scale
        assert ref.o.shape == want.shape
        assert float((ref.o - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max()))
        assert bool((ref.S >= ref.o.abs()).all()) and bool((ref.prod <= ref.S).all())


def test_conv_ref64_on_gaussian_inputs_with_silu():
    """the same agreement away from the integers: Gaussian operands, the SiLU of the fused norm, odd sizes, upsample, concat"""
    gen = torch.Generator().manual_seed(3)
    rn = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)
    x1, x2, w, b, bnc, res = rn(2, 5, 3, 7), rn(2, 3, 3, 7), rn(6, 8, 3, 3), rn(6), rn(2, 6), rn(2, 6, 6, 14)
    ga, gb = rn(2, 8), rn(2, 8)
    ref = R.conv_ref64(x1, x2, w, b, bnc, res, True, 0.7, gn=(ga, gb, True))
    x = F.silu(torch.cat([x1, x2], 1) * ga[:, :, None, None] + gb[:, :, None, None])
    want = (F.conv2d(F.interpolate(x, scale_factor=2, mode='nearest'), w, b, padding=1) + bnc[:, :, None, None] + res) * 0.7
    assert float((ref.o - want).abs().max()) < 1e-12


def test_strip_statistics_layout():
    o = torch.arange(2 * 3 * 8 * 16, dtype=torch.float64).reshape(2, 3, 8, 16)
    st = R.strip_stats64(o)
    assert tuple(st.shape) == (4, 3, 2)
    v = o.permute(0, 2, 3, 1).reshape(256, 3)
    assert torch.equal(st[1, :, 0], v[64:128].sum(0)) and torch.equal(st[3, :, 1], (v[192:] ** 2).sum(0))
    assert torch.equal(R.image_stats64(o), st.view(2, 2, 3, 2).sum(1))


@pytest.mark.parametrize('name,mode', CASE_MODE)
def test_every_launch_is_inside_the_exactness_conditions(name, mode):
    case = CASES[name]
    ho, wo = R.out_hw(case)
    for variant in case.variants:
        if variant != 'int' and mode not in R.W32:
            continue
        a, ref = _args_ref(name, mode, variant)
        stats = None
        if case.stats and variant == 'int' and (ho * wo) % 64 == 0:
            stored = ref.o.to(_out_dtype(case, mode)).double()
            stats = R.image_stats64(stored) if case.form.startswith('pp') else R.strip_stats64(stored)
        R.assert_exact_conditions(ref, _out_dtype(case, mode), stats, a)
        assert float(ref.o.abs().max()) > 0
        if variant == 'x_lo':       # the lo plane is not empty; beside an integer the hi part is that integer
            hi, big = a['x1'].to(torch.float16).double(), a['x1'].abs() > 0.5
            assert bool((hi != a['x1']).any()) and torch.equal(hi[big], a['x1'].round()[big])
        if variant == 'w_lo':
            assert bool((a['w'].to(torch.float16).double() != a['w']).any())
        if case.split2:             # hi + lo == 64 * o with hi the float16 rounding: both halves are float16 numbers
            hi = (64 * ref.o).to(torch.float16).double()
            assert R.representable(64 * ref.o - hi, torch.float16) and bool((64 * ref.o != hi).any())


def test_the_route_table_is_complete():
    """every (kernel form) x (mode) cell has a case or a one-line reason, never both; the grids of the implicit-GEMM cases reach the block
    counts that are no multiple of 8; every launch costs well under 1.5 GFLOP of float64"""
    have = {(c.form, m) for c in CASES.values() for m in c.modes}
    for form in FORMS:
        for mode in MODES:
            assert ((form, mode) in have) != ((form, mode) in ABSENT), (form, mode)
    assert all(isinstance(r, str) and r for r in ABSENT.values())
    blocks = {R.igemm_blocks(c, 'bf16') for c in CASES.values() if c.form == 'igemm' and 'bf16' in c.modes}
    assert {1, 3, 7, 9, 13} <= blocks, sorted(blocks)
    ups = [c for c in CASES.values() if c.form == 'igemm' and c.up]
    assert any(c.h % 2 and c.w % 2 for c in ups) and any(c.c2 for c in ups) and any('r' in c.ep for c in ups) and any(c.k == 1 for c in ups)
    assert all(c.up for c in CASES.values() if c.name.startswith('up_') or '_up' in c.name)
    # the K split, implicit-GEMM kernel: the reduce pass is instantiated per slab count 2..8, and every one of them is reached -- by the
    # plain reduce kernel and, at 4, 5 and 8 (the counts no other case has), by the one that writes the strip statistics too
    ig = [c for c in CASES.values() if c.form == 'igemm_splitk']
    assert {R.effective_splits(c, m)[0] for c in ig for m in c.modes} == set(range(2, 9))
    with_stats = lambda c: c.stats and (R.out_hw(c)[0] * R.out_hw(c)[1]) % 64 == 0
    for want in (False, True):
        assert {R.effective_splits(c, m)[0] for c in ig for m in c.modes if with_stats(c) == want} >= {2, 3, 4, 5, 8}, want
    assert {R.effective_splits(c, m)[0] for c in CASES.values() if c.form == 'pp_splitk' for m in c.modes} >= {2, 3, 5, 8}
    # the cases that exist to pass a grid cap (SIZE_LOOPS below) cost what their cap makes them cost; every other launch stays cheap
    sized = {name for name, *_ in SIZE_LOOPS if R.small_trips(CASES[name], CASES[name].modes[0]).trips > 1} | {'split2_reduce_2trips'}
    assert set(R.LARGE) <= sized
    for c in CASES.values():
        ho, wo = R.out_hw(c)
        assert 2.0 * c.n * ho * wo * c.cout * c.k * c.k * (c.c1 + c.c2) < (4e9 if c.name in sized else 1.5e9), c.name
        assert all(k in ('conv_tile', 'conv_waves', 'conv_stages', 'conv_epi32', 'conv_splits', 'conv_variant') for k, _ in c.knobs)
        if 'N' in c.ep:
            assert c.n >= 2, 'a wider bias_nc shows only from the second sample on'
        # which epilogue runs is pinned: unsplit by conv_splits = 1, or a forced split that the launcher honours in every mode
        assert dict(c.knobs).get('conv_splits') == (c.splits if c.splits > 0 else None), c.name
        if c.splits > 1:
            assert all(R.effective_splits(c, m)[0] > 1 for m in c.modes), c.name
        if c.splits == 0:
            assert c.skip is not None or c.form.startswith('in3') or c.form.startswith('out3'), c.name
    assert sum(c.splits == -1 for c in CASES.values()) == 2          # the launchers' own estimate: one case per kernel
    # no case claims a knob form that does not exist (conv_reference.KNOB_ABSENT)
    for c in CASES.values():
        kn = dict(c.knobs)
        assert not ({'conv_waves', 'conv_stages'} & set(kn) and 'f32' in c.modes), c.name
        assert not (kn.get('conv_stages') == 4 and ('f16x3' in c.modes or kn.get('conv_waves') == 8)), c.name
        assert not ('conv_epi32' in kn and set(c.modes) & set(R.H16)), c.name
    # the row-layout epilogue's forms are reached: f32 with epi32 = 1 on whole strips, an out_split2 output under every value
    assert any(dict(c.knobs).get('conv_epi32') == 1 and 'f32' in c.modes and (c.h * c.w) % 64 == 0 and c.splits == 1 for c in CASES.values())
    assert {dict(c.knobs).get('conv_epi32') for c in CASES.values() if c.split2 and (c.h * c.w) % 64 == 0} >= {0, 1, 2}
    # a launch asked for statistics it cannot give
    assert any(c.stats and (R.out_hw(c)[0] * R.out_hw(c)[1]) % 64 for c in CASES.values())


# ---- loops whose trip count the launcher derives from the size ------------------------------------------------------------------------
# (case, units the loop walks, segments per wave, blocks, most trips of a thread, units left for the last trip): the numbers the comments of
# conv_reference.py state, here from its restatement of the launchers' rules (small_trips).  A changed cap or segments-per-wave rule in
# conv_small.hip must be restated there, and then fails HERE unless the shapes still pass it.
SIZE_LOOPS = [
    ('in3_mfma_67x992', 4154, 2, 520, 2, 2074),                 # 2080 waves: 2074 take a second segment, 6 take one
    ('in3_mfma_260x4048', 65780, 8, 2048, 9, 244),              # 2056 blocks asked for, 2048 given: a ninth trip for 244 waves
    ('in3_direct_928x1130_c8', 1048640, None, 4096, 2, 64),     # cap 4096 * 256 = 1,048,576, + 64
    ('out3_direct_464x1130_c8', 524320, None, 8192, 2, 32),     # cap 8192 * 64 = 524,288, + 32
]


def test_first_and_last_convolution_routes_and_trip_counts():
    """every in3 / out3 case takes the kernel its form names, in every mode; the size-driven loops make the trips the table says; every OTHER
    case makes exactly one (so the table is the whole multi-trip coverage); the ragged staging groups of conv_in3_kernel are reached"""
    small = [c for c in CASES.values() if c.form.startswith('in3') or c.form.startswith('out3')]
    for c in small:
        for m in c.modes:
            assert R.small_route(c, m) == c.form, (c.name, m)
    table = {row[0]: row[1:] for row in SIZE_LOOPS}
    for c in small:
        for m in c.modes:
            t = R.small_trips(c, m)
            if c.name in table:
                units, spw, blocks, trips, last = table[c.name]
                assert (t.units, t.per_wave, t.blocks, t.trips) == (units, spw, blocks, trips), (c.name, t)
                assert t.units - (trips - 1) * t.per_pass == last and 0 < last < t.per_pass, (c.name, t)
                assert t.last_start == (trips - 1) * t.per_pass * (16 if c.form == 'in3_mfma' else 1)       # (a segment is 16 pixels)
            else:
                assert t.trips == 1, (c.name, t)
    # the cap is passed by less than a block's worth of a wave each: the smallest shapes that take the trip
    assert R.small_trips(CASES['in3_direct_928x1130_c8'], 'f32').units - 4096 * 256 == 64
    assert R.small_trips(CASES['out3_direct_464x1130_c8'], 'f32').units - 8192 * 64 == 32
    assert 65780 // 2048 >= 8 and -(-65780 // 32) == 2056 > 2048
    # conv_in3_kernel's staging groups: whole groups in the older cases, ragged ones (5; 8 + 2) at cout 40, a single short group at cout 8
    groups = {(c.name, m): R.in3_direct_groups(c, m) for c in small if c.form == 'in3_direct' for m in c.modes}
    assert groups[('in3_direct_12x20_c40', 'bf16')] == [5] and groups[('in3_direct_12x20_c40', 'f16')] == [5]
    assert groups[('in3_direct_12x20_c40', 'f32')] == [8, 2]
    assert all(g == [8] * len(g) for (name, _), g in groups.items() if CASES[name].cout in (64, 128, 192))
    # the bias of the unaligned case is what keeps it off the matrix-core kernel
    c = CASES['in3_direct_16x16_unaligned_bias']
    assert R.small_route(c._replace(ep='b'), 'f32') == 'in3_mfma' and R.small_route(c, 'f32') == 'in3_direct'
    # c = 48 at 16 x 16: tiled in f32 (three chunks of 16), direct in 16-bit
    assert R.small_route(CASES['out3_tiled_16x16_c48'], 'f32') == 'out3_tiled' and CASES['out3_tiled_16x16_c48'].c1 // 16 == 3
    assert all(R.small_route(CASES['out3_tiled_16x16_c48'], m) == 'out3_direct' for m in R.H16)


def test_the_reduce_pass_takes_its_second_trip():
    """conv_splitk_reduce_kernel's grid-stride loop: 524,400 threads' worth against 2048 blocks of 256; every other split case makes one
    trip; two slabs fit the workspace; the split is honoured in every mode"""
    c = CASES['split2_reduce_2trips']
    for m in c.modes:
        t = R.reduce_trips(c, m)
        assert (t.units, t.blocks, t.trips, t.units - t.per_pass) == (524400, 2048, 2, 112)
        assert t.last_start == 32768 and 32775 - t.last_start == 7
        assert R.effective_splits(c, m)[0] == 2
    assert (75 * 437) % 64 != 0, 'whole strips would send a statistics request to the other reduce kernel'
    assert 2 * 32775 * 64 * 4 < 96 << 20
    for o in CASES.values():
        if o.splits > 1 and o.name != c.name:
            assert all(R.reduce_trips(o, m).trips == 1 for m in o.modes), o.name


@pytest.mark.parametrize('name', [row[0] for row in SIZE_LOOPS] + ['split2_reduce_2trips'])
def test_the_last_trip_writes_nonzero_values(name):
    """what the last trip of a size-driven loop writes is not all zero in the reference (in every pixel; in every group of 4 couts of every
    pixel for the reduce pass: one thread's float4), so a launch that skipped the trip cannot equal it; and the case stays inside the exactness
    conditions with room (S <= 85 on the 3- and 8-channel inputs, where nearly every activation is nonzero)"""
    case = CASES[name]
    for mode in case.modes:
        a, ref = _args_ref(name, mode)
        last = R.last_trip_values(case, mode, ref.o)
        t = R.small_trips(case, mode) if case.splits == 0 else R.reduce_trips(case, mode)
        assert last.shape[0] == case.n * R.out_hw(case)[0] * R.out_hw(case)[1] - t.last_start > 0
        nz = int((last != 0).sum())
        print(f'{name} [{mode}]: last trip writes {last.numel()} elements, {nz} nonzero; max S {float(ref.S.max())}')
        per_thread = last.reshape(-1, 4) if case.splits > 1 else last          # (the small kernels: a thread or a wave owns whole pixels)
        assert bool((per_thread != 0).any(1).all()), 'what one thread writes in the last trip is all zero'
        assert 2 * nz > last.numel()
        if case.splits == 0:
            assert float(ref.S.max()) <= 85.0
        del a, ref, last


# ---- teeth: mistakes a kernel could make, made HERE on the reference's own steps ----------------------------------------------------
def _applies(fault, case):
    conv2d = not (case.form.startswith('in3') or case.form.startswith('out3'))
    return {
        'tap_shift': case.k == 3,
        'kh_kw': case.k == 3 and case.h * case.w > 1,          # (a 1x1 image meets the centre tap only)
        'concat_swap': case.c2 > 0,
        'last_chunk': conv2d and case.c1 + case.c2 >= 128,
        'up_index': case.up,
        'pad_first': case.gn,
        'last_split': case.splits > 1,
        'bias_nc_ld': 'N' in case.ep,
    }[fault]


FAULTS = ('tap_shift', 'kh_kw', 'concat_swap', 'last_chunk', 'up_index', 'pad_first', 'last_split', 'bias_nc_ld')


def _tap_sums_unchecked_border(x, w):
    """R.tap_sums with the right-border check of tap (1, 2) and the bottom-border check of tap (2, 1) missing: there the tap reads the
    pixel itself instead of the padding"""
    n, c, h, wd = x.shape
    xp = torch.zeros(n, c, h + 2, wd + 2, dtype=torch.float64)
    xp[:, :, 1:-1, 1:-1] = x
    o = torch.zeros(n, w.shape[0], h, wd, dtype=torch.float64)
    for kh in range(3):
        for kw in range(3):
            xs = xp[:, :, kh:kh + h, kw:kw + wd].clone()
            if (kh, kw) == (1, 2):
                xs[:, :, :, wd - 1] = x[:, :, :, wd - 1]
            if (kh, kw) == (2, 1):
                xs[:, :, h - 1, :] = x[:, :, h - 1, :]
            o += torch.einsum('oc,nchw->nohw', w[:, :, kh, kw], xs)
    return o, torch.zeros_like(o)


def _tap_sums_of_padded(xp, w):
    """the nine taps over an input that already carries its border"""
    h, wd = xp.shape[2] - 2, xp.shape[3] - 2
    o = torch.zeros(xp.shape[0], w.shape[0], h, wd, dtype=torch.float64)
    for kh in range(3):
        for kw in range(3):
            o += torch.einsum('oc,nchw->nohw', w[:, :, kh, kw], xp[:, :, kh:kh + h, kw:kw + wd])
    return o, torch.zeros_like(o)


def _faulty(fault, case, mode, a):
    """the output of the reference's steps with one mistake in them"""
    x1, x2, w, bias_nc = a['x1'], a['x2'], a['w'].double(), a['bias_nc']
    x = R.prepare_input(x1, x2, a['gn'], case.up)
    sums = R.tap_sums
    if fault == 'tap_shift':
        sums = _tap_sums_unchecked_border
    elif fault == 'kh_kw':
        w = w.transpose(2, 3)
    elif fault == 'concat_swap':
        x = R.prepare_input(x2, x1, a['gn'], case.up)
    elif fault == 'last_chunk':                     # the last 64-channel chunk of K never accumulated
        w = w.clone()
        w[:, -64:] = 0
    elif fault == 'last_split':                     # the last K split never added by the reduce pass
        w = w * R.last_split_mask(case, mode).permute(2, 0, 1)[None].double()
    elif fault == 'up_index':                       # source index (h + 1) >> 1 instead of h >> 1 (kept inside the image)
        src = R.prepare_input(x1, x2, a['gn'], False)
        ih = ((torch.arange(2 * case.h) + 1) >> 1).clamp(max=case.h - 1)
        iw = ((torch.arange(2 * case.w) + 1) >> 1).clamp(max=case.w - 1)
        x = src[:, :, ih][:, :, :, iw]
    elif fault == 'pad_first':                      # the zero border laid before the norm: the border taps see act(b) instead of 0
        raw = R.prepare_input(x1, x2, None, False)
        xp = torch.zeros(raw.shape[0], raw.shape[1], raw.shape[2] + 2, raw.shape[3] + 2, dtype=torch.float64)
        xp[:, :, 1:-1, 1:-1] = raw
        x, sums = R.norm_input(xp, a['gn']), _tap_sums_of_padded
    elif fault == 'bias_nc_ld':                     # the column slice read with the row stride of a dense [n, cout] tensor
        flat = a['bias_nc_wide'].reshape(-1)
        bias_nc = flat[case.cout:case.cout + case.n * case.cout].reshape(case.n, case.cout)
    else:
        raise KeyError(fault)
    o, s = sums(x, w)
    assert a['skip'] is None
    return R.epilogue(o, s, a['bias'], bias_nc, a['residual'], a['out_scale'])


@pytest.mark.parametrize('fault', FAULTS)
def test_the_net_has_teeth(fault):
    """each mistake shows in at least one output element of EVERY case (and mode granule) it applies to"""
    hit = 0
    for name, mode in CASE_MODE:
        case = CASES[name]
        if case.skip is not None or not _applies(fault, case) or (fault != 'last_split' and mode != case.modes[0]):
            continue
        a, ref = _args_ref(name, mode)
        bad = _faulty(fault, case, mode, a)
        differ = int((bad.o != ref.o).sum())
        print(f'{fault}: {name} [{mode}] {differ} of {ref.o.numel()} elements differ')
        assert differ > 0, (fault, name, mode)
        hit += 1
    assert hit >= 2, f'{fault} applies to {hit} cases'
