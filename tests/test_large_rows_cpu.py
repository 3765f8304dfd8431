"""CPU: the case table of the large-batch GPU tests (launch_rules.LARGE_CASES) and the machinery they rest on (tests/large_rows.py), held to
account without a GPU.

  - every tensor's bytes and boundary crossings are recomputed from the shapes; behind the last boundary a tensor crosses lie at least 7 whole
    samples;
  - the seeded map: the samples that hold byte 2^31 / byte 2^32 / element 2^31 of a tensor have another base than sample 0 and than the samples a
    lost bit 31 / 32 would displace them to, so a systematic shift cannot pass by coincidence;
  - every dts_conv2d case's route through dts_conv_plan (launch-free): kernel, tile, splits == 1, who writes the statistics;
  - the switch at 2^31 bytes and the refusal at 2^30 pixels, from both sides (launch-free queries only: nothing here or on the GPU calls a
    launching entry point with sizes its buffers do not back);
  - the comparison itself fails when it must: a row swapped for another class's row, one element changed in a row that -- at the sample size of
    a real case -- lies beyond 2^32 bytes."""
import ctypes as C
import os
import sys

import pytest
import torch

import large_rows as LG
import launch_rules as LR
from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, 'tools'))
import conv_plan_sweep as S  # noqa: E402

CASES = list(LR.LARGE_CASES.values())
CODE = {'31': 'byte31', '32': 'byte32', 'e31': 'elem31'}


@pytest.mark.parametrize('case', CASES, ids=lambda c: c.name)
def test_case_crosses_what_it_claims(case):
    assert case.n >= LG.K
    crossed = set()
    for t in case.tensors:
        sample_bytes = LG.numel(t.sample_shape) * t.itemsize
        assert t.bytes == case.n * sample_bytes, t.name
        assert tuple(CODE[c] for c in t.crosses) == LG.crossings(t.bytes, t.itemsize), t.name
        for b in LG.crossings(t.bytes, t.itemsize):
            assert LG.samples_beyond(case.n, sample_bytes, LG.boundary_byte(b, t.itemsize)) >= 7, (t.name, b)
            crossed.add(b)
    assert 'byte31' in crossed, 'a large case crosses 2^31 bytes in at least one tensor'
    # what one launch holds at once (inputs, outputs; the routes of a GroupNorm case run one after the other) stays under 16 GiB
    alive = sum(t.bytes for t in case.tensors if not t.name.startswith('out_')) if case.family == 'groupnorm' else sum(t.bytes for t in case.tensors)
    assert alive <= 16 << 30, alive


def test_table_names_every_boundary_for_every_family():
    for family in {c.family for c in CASES}:
        crossed = {b for c in CASES if c.family == family for t in c.tensors for b in t.crosses}
        assert {'31', '32'} <= crossed, (family, crossed)


@pytest.mark.parametrize('case', CASES, ids=lambda c: c.name)
def test_map_separates_the_samples_at_the_boundaries(case):
    idx = LG.row_map(case.n)
    assert idx.dtype == torch.int64 and tuple(idx.shape) == (case.n,) and int(idx.min()) == 0 and int(idx.max()) == LG.K - 1
    assert not torch.equal(idx, torch.arange(case.n) % LG.K)
    assert torch.equal(idx, LG.row_map(case.n)), 'seeded: the same map every time'
    for t in case.tensors:
        sample_bytes = LG.numel(t.sample_shape) * t.itemsize
        assert LG.map_separates(idx, case.n, sample_bytes, t.itemsize) == [], t.name


def test_map_separates_notices_a_periodic_map():
    """what the property is for: a map under which the sample at byte 2^32 has the base of the sample 2^32 bytes before it (sample 0) would let
    an offset that lost bit 32 pass"""
    n, sample_bytes = (1 << 17) + 7, 1 << 15                  # wrap distance 2^32 / 2^15 = 2^17 samples
    assert LG.wrap_distances(sample_bytes, 2)[0] == 1 << 17
    idx = LG.row_map(n)
    assert LG.map_separates(idx, n, sample_bytes, 2) == []
    idx[1 << 17] = idx[0]
    assert LG.map_separates(idx, n, sample_bytes, 2) != []
    idx = torch.arange(n) % LG.K                              # the periodic map: the sample at byte 2^31 (65536 = 7 * 9362 + 2) and its image 65536
    idx[0] = idx[1 << 16]                                     # samples on share a base as soon as the period divides the distance; here by hand
    assert LG.map_separates(idx, n, sample_bytes, 2) != []


# ---- dts_conv2d: the route of every case, the switch at the limits --------------------------------------------------------------------------
def _plan(lib, L, mode, n, h, w, c1, cout, k, up=0, res=0, gn=0, stats=0, bias_nc=0):
    ca, info = S.conv_args(L, S.row(S.MODE[mode], n, h, w, c1, cout, k, 0, up, res, gn, stats)[0]), L.ConvPlanInfo()
    if bias_nc:
        ca.bias_nc, ca.ld_bias_nc = 0x1000, cout
    st = lib.dts_conv_plan(C.byref(ca), C.byref(info))
    kernel = lib.dts_conv_kernel(C.byref(ca))
    return st, info, kernel, lib.dts_last_error().decode()


@pytest.fixture(scope='module')
def lib():
    from diffusion_tts_amd import _lib as L
    lib = L.load()
    old = {k: int(lib.dts_get_tuning(L.KNOBS[k])) for k in S.CONV_KNOBS}
    S.set_knobs(L, lib, {})
    yield lib, L
    S.set_knobs(L, lib, {k: v for k, v in old.items() if v != -1})


CONV2D = [c for c in CASES if c.family == 'conv2d']


@pytest.mark.parametrize('case', CONV2D, ids=lambda c: c.name)
def test_conv2d_case_route(lib, case):
    lib, L = lib
    s = case.spec
    st, info, kernel, err = _plan(lib, L, s['mode'], case.n, s['h'], s['w'], s['c1'], s['cout'], s['k'], s['up'], 'r' in s['ep'], s['gn'], s['stats'], 'n' in s['ep'])
    assert st == 0 and info.refused == 0, err
    assert kernel == info.kernel
    want = dict(s['plan'], splits=1)
    if s['stats']:
        want.update(stats_in_reduce=0, stats_written=1)
    else:
        want.update(stats_in_kernel=0, stats_in_reduce=0, stats_written=0)
    got = {f: int(getattr(info, f)) for f in want}
    assert got == want, (case.name, got, want)
    if s['gn']:
        assert info.fuses_gn == 1
    if s['up'] == 2:          # the phase form: the query that gates the weight form says yes for exactly these arguments
        ca = S.conv_args(L, S.row(S.MODE[s['mode']], case.n, s['h'], s['w'], s['c1'], s['cout'], s['k'], 0, 2, 'r' in s['ep'], 0, 0)[0])
        assert lib.dts_conv_takes_phases(C.byref(ca)) == 1


def test_conv2d_table_covers_the_routes():
    kinds = {(c.spec['mode'], c.spec['plan']['kernel'], c.spec['k'], c.spec['up']) for c in CONV2D}
    for need in (('bf16', 0, 1, 0), ('f16', 0, 3, 0), ('bf16', 6, 3, 0), ('f16', 6, 3, 0), ('f16x3', 0, 3, 0), ('f32', 0, 3, 0), ('bf16', 0, 3, 1),
                 ('f16', 0, 3, -1), ('f16x3', 0, 3, 2)):
        assert need in kinds, need
    assert any('n' in c.spec['ep'] for c in CONV2D) and any(c.spec['gn'] for c in CONV2D) and any(c.spec['stats'] and 'r' in c.spec['ep'] for c in CONV2D)


def test_switch_at_the_limits_from_both_sides(lib):
    lib, L = lib
    sw = LR.LARGE_CONV_SWITCH
    shape = (sw['h'], sw['w'], sw['c1'], sw['cout'], sw['k'])
    n_pp, k_pp = sw['last_pp']
    n_ig, k_ig = sw['first_igemm']
    assert n_ig == n_pp + 1
    assert n_pp * sw['h'] * sw['w'] * sw['c1'] * 2 == (1 << 31) - 32768 and n_ig * sw['h'] * sw['w'] * sw['c1'] * 2 == 1 << 31
    st, info, kernel, err = _plan(lib, L, sw['mode'], n_pp, *shape)
    assert (st, info.refused, info.kernel, kernel, info.splits) == (0, 0, k_pp, k_pp, 1), err
    st, info, kernel, err = _plan(lib, L, sw['mode'], n_ig, *shape)
    assert (st, info.refused, info.kernel, kernel, info.splits) == (0, 0, k_ig, k_ig, 1), err
    assert info.tile == 192
    # 2^30 pixels
    assert sw['first_refused'] * sw['h'] * sw['w'] == 1 << 30 and sw['last_accepted'] == sw['first_refused'] - 1
    st, info, kernel, err = _plan(lib, L, sw['mode'], sw['last_accepted'], *shape)
    assert (st, info.refused, info.kernel, kernel) == (0, 0, 0, 0), err
    st, info, kernel, err = _plan(lib, L, sw['mode'], sw['first_refused'], *shape)
    assert st != 0 and info.refused == 1 and sw['refusal'] in err and kernel < 0, (st, err, kernel)


# ---- the comparison fails when it must ---------------------------------------------------------------------------------------------------------
def _tiled(n=4099, m=24, dtype=torch.float32, seed=3):
    base = torch.randn(LG.K, m, generator=torch.Generator().manual_seed(seed)).to(dtype)
    base[2, 5] = float('nan')            # a NaN the "kernel" produces in every row of class 2: bits compare equal
    base[3, 0], base[4, 0] = 0.0, 0.0
    idx = LG.row_map(n, seed=5)
    return base, idx, LG.tile(base, idx)


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16, torch.float16, torch.float64, torch.uint8])
def test_identical_classes_pass(dtype):
    base, idx, out = _tiled(dtype=torch.float32)
    out = (out.nan_to_num(1.0) * 16).to(dtype) if dtype == torch.uint8 else out.to(dtype)
    for chunk in (1, 1000, 64 << 20):
        assert LG.class_mismatches(out, idx, chunk_bytes=chunk) == []
    LG.assert_classes_bit_equal(out, idx)
    assert torch.equal(LG.first_of_classes(out, idx)[:, 1], out[LG.first_rows(idx), 1])


def test_a_row_swapped_for_another_class_fails():
    base, idx, out = _tiled()
    r = 3000
    other = (int(idx[r]) + 1) % LG.K
    out[r] = base[other]
    bad = LG.class_mismatches(out, idx, chunk_bytes=4096)
    assert [b[:2] for b in bad] == [(r, int(idx[r]))]
    with pytest.raises(AssertionError):
        LG.assert_classes_bit_equal(out, idx)


def test_one_element_changed_beyond_4_gib_fails():
    """a stand-in of 24 floats per row; at the sample size of a real case (32 KiB) the changed row lies beyond byte 2^32.  Every chunking finds
    it, in the last rows of the tensor and at both ends of a chunk, and a flipped sign of zero counts (bits, not values)."""
    base, idx, out = _tiled(n=131079)
    sample_bytes = 32768
    for r, e in ((131075, 23), (131072, 0), (131078, 11)):
        assert LG.sample_at_byte(LG.B32, sample_bytes) <= r and r * sample_bytes >= LG.B32
        t = out.clone()
        t[r, e] = torch.nextafter(t[r, e], torch.tensor(float('inf'))) if not bool(torch.isnan(t[r, e])) else 0.0
        for chunk in (96, 24 * 4 * 1000, 64 << 20):
            bad = LG.class_mismatches(t, idx, chunk_bytes=chunk)
            assert bad == [(r, int(idx[r]), e)], (r, e, chunk, bad)
    zrow = int(((idx == 3) & (torch.arange(len(idx)) > 131072)).nonzero()[0])
    t = out.clone()
    t[zrow, 0] = -0.0
    assert LG.class_mismatches(t, idx) == [(zrow, 3, 0)]


def test_the_first_row_of_a_class_is_not_exempt():
    """the first row is the class's reference: if IT is the wrong one, every other row of the class differs from it"""
    base, idx, out = _tiled(n=500)
    f = int(LG.first_rows(idx)[1])
    out[f, 7] += 1.0
    bad = LG.class_mismatches(out, idx, limit=1 << 30)
    assert len(bad) == int((idx == 1).sum()) - 1 and all(b[1] == 1 and b[2] == 7 for b in bad)


def test_guard_bands():
    for dtype in (torch.float32, torch.bfloat16, torch.uint8):
        buf, view = LG.guarded((5, 3, 2), dtype, 'cpu')
        assert tuple(view.shape) == (5, 3, 2) and view.data_ptr() == buf.data_ptr() + LG.GUARD * buf.element_size()
        assert LG.bands_intact(buf)
        view.fill_(1)
        assert LG.bands_intact(buf)
        buf[LG.GUARD - 1] = 1
        assert not LG.bands_intact(buf)
        buf, view = LG.guarded((4,), dtype, 'cpu')
        buf[-LG.GUARD] = 1
        assert not LG.bands_intact(buf)


def test_byte_bookkeeping():
    assert LG.crossings(LG.B31, 2) == () and LG.crossings(LG.B31 + 1, 2) == ('byte31',)
    assert LG.crossings(LG.B32 + 2, 2) == ('byte31', 'byte32', 'elem31') and LG.crossings(LG.B32 + 4, 4) == ('byte31', 'byte32')
    assert LG.crossings(2 * LG.B32 + 4, 4) == ('byte31', 'byte32', 'elem31')
    assert LG.sample_at_byte(LG.B32, 32768) == 131072 and LG.sample_at_byte(LG.B32, 98304) == 43690
    assert LG.samples_beyond(131079, 32768, LG.B32) == 7 and LG.samples_beyond(43698, 98304, LG.B32) == 7
    assert LG.wrap_distances(32768, 2) == [131072, 262144, 65536] and LG.wrap_distances(98304, 2) == []


# ---- the kernels with documented caps: the cap from both sides where a launch-free query exists ---------------------------------------------
def test_jpeg_size_case_sits_at_the_cap(lib):
    """dts_jpeg_workspace_bytes answers 0 for a shape dts_jpeg_size refuses: the case is the last n it takes at 128 x 128 (n * 384 blocks <= 2^24),
    its workspace passes 2^32 bytes and its bit buffer -- 256 bytes per block, what the cap is for -- ends below 2^32"""
    lib, L = lib
    lib.dts_jpeg_workspace_bytes.restype = C.c_int64
    case = LR.LARGE_CASES['jpeg_size_cap']
    h, w, n = case.spec['h'], case.spec['w'], case.n
    lay = LR.jpeg_layout(n, h, w)
    assert n * lay.nb <= case.spec['cap_blocks'] < (n + 1) * lay.nb and n <= 65535
    assert LR.jpeg_shape_ok(n, h, w) and not LR.jpeg_shape_ok(n + 1, h, w)
    assert int(lib.dts_jpeg_workspace_bytes(n, h, w)) == lay.bytes and int(lib.dts_jpeg_workspace_bytes(n + 1, h, w)) == 0
    assert lay.bitbuf < LG.B32 < lay.bytes and lay.bytes - lay.bitbuf == n * lay.nb * LR.JPEG_BLOCK_BUF_BYTES < LG.B32


def test_group_rows_case_sits_at_the_cap():
    from diffusion_tts_amd import ops
    case = LR.LARGE_CASES['group_rows_cap']
    assert case.n == case.spec['cap_rows'] == ops.GROUP_ROWS_MAX
    row_bytes = LG.numel(case.tensors[0].sample_shape) * 4
    assert row_bytes % 16 == 0 and (case.n - 7) * row_bytes >= LG.B32 > (case.n - 8) * row_bytes
