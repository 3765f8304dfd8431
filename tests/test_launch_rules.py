"""CPU: the tables of tests/launch_rules.py against its restatement of the launchers' rules -- each case that exists to take the second
trip of a size-driven loop does take it, by the margin its comment states.  No GPU and, but for one host-only size query (the JPEG workspace), nothing of
the library: if a cap or a heuristic changes there, the restatement has to follow, and these assertions then say which cases lost their
coverage."""
import pytest

import launch_rules as L


@pytest.mark.parametrize('case', L.XATTN_CHUNK_LOOP, ids=lambda c: f'n{c.n}-h{c.heads}-d{c.d}-tq{c.tq}')
def test_cross_attention_cases_walk_several_chunks(case):
    assert L.xattn_plan(case.n, case.heads, case.tq) == (case.chunks, case.qchunks, case.qblocks)
    assert case.qchunks > 1 and case.tq % 64 != 0
    assert case.qchunks * case.qblocks > case.chunks, 'the last block has no chunk past the end: the break is not taken'
    assert 1 <= case.tk <= 128 and case.d in (64, 128, 256)


def test_cross_attention_chunk_counts_covered():
    """qchunks 2, 4 and 8 are all reached (8 is what the SD U-Net runs at 16 candidates: n * heads = 128, tq = 4096); the shapes of the older
    tests (n = 2, heads = 2; n = 6, heads = 8) stay at 1"""
    assert {c.qchunks for c in L.XATTN_CHUNK_LOOP} == {2, 4, 8}
    assert L.xattn_plan(16, 8, 4096)[1] == 8
    assert all(L.xattn_plan(2, 2, tq)[1] == 1 for tq in (1, 64, 4096)) and L.xattn_plan(6, 8, 100)[1] == 1
    assert sum(c.tk == 128 for c in L.XATTN_CHUNK_LOOP) == 1 and sum(c.contexts is not None for c in L.XATTN_CHUNK_LOOP) == 1
    assert any(c.d == 256 for c in L.XATTN_CHUNK_LOOP)


GN_ALL = {**L.GN_ROWS_TWO_TRIPS, **L.GN_GRID_TWO_TRIPS}


@pytest.mark.parametrize('name', list(GN_ALL))
def test_group_norm_apply_cases_take_the_second_trip(name):
    c = GN_ALL[name]
    for dt in c.dtypes:
        plan = L.gn_apply_plan(c.n, c.c1, c.c2, c.h, c.w, dt == 'f32', c.pool)
        for field, want in c.expect.items():
            assert getattr(plan, field) == want, (name, dt, field, plan)
        assert plan.trips == 2
        if plan.kernel == 'grid':       # past the cap by less than one block
            assert 0 < plan.threads - L.GN_GRID_CAP * 256 < 256


def test_group_norm_apply_instantiations():
    """the split-image forms of the row kernel (<float, SPLIT> and <float, SPLIT, W16>) and of the grid-stride kernel (<float, POOL, SPLIT>)"""
    c = L.GN_ROWS_TWO_TRIPS['c192']
    assert L.gn_apply_plan(c.n, c.c1, c.c2, c.h, c.w, True, split=True).w16 is True
    assert L.gn_apply_plan(c.n, c.c1, c.c2, c.h, c.w, True, split=True, gn_fuse=2).w16 is False
    o = L.GN_ROWS_TWO_TRIPS['c100+92']
    assert o.c1 % 8 != 0 and o.c1 % 4 == 0 and (o.c1 + o.c2) % 32 == 0
    assert L.gn_apply_plan(o.n, o.c1, o.c2, o.h, o.w, True, split=True).w16 is False
    assert L.gn_apply_plan(2, 192, 0, 50, 874, True, pool=True, split=True).kernel == 'grid'
    assert L.gn_apply_plan(1, 1536, 0, 1, 2731, True, split=True).kernel == 'grid'
    # the production shape the issue names: 128 x 64 x 64 at C = 192 makes 13 pair trips
    assert L.gn_apply_plan(128, 192, 0, 64, 64, True).trips == 13
    # the largest shapes of the older tests: one trip each
    assert L.gn_apply_plan(2, 192, 0, 64, 64, True).trips == 1 and L.gn_apply_plan(2, 192, 0, 64, 64, True, pool=True).trips == 1
    assert L.gn_apply_plan(2, 1536, 0, 6, 10, True).kernel == 'grid' and L.gn_apply_plan(2, 1536, 0, 6, 10, True).trips == 1


def test_layer_norm_widths():
    for c, want in L.LAYER_NORM_WIDTHS.items():
        assert L.layer_norm_vectors(c) == want and c % 8 == 0 and c <= 2048
    assert all(L.layer_norm_vectors(c)[0] <= 3 for c in (64, 128, 320, 1024, 1280))      # the older widths never reach the fourth vector


# ---- dts_jpeg_size --------------------------------------------------------------------------------------------------------------------------
def test_jpeg_scan_shapes_take_every_form_of_the_per_thread_loop():
    for (h, w), (nb, per, busy, last) in L.JPEG_SCAN_SHAPES.items():
        assert L.jpeg_layout(1, h, w).nb == nb and L.jpeg_scan_plan(nb) == (per, busy, last), (h, w)
        assert (busy - 1) * per + last == nb and 1 <= last <= per and busy <= 256
    plans = set(v[1:] for v in L.JPEG_SCAN_SHAPES.values())
    assert {p[0] for p in plans} >= {1, 2, 3, 4, 24}
    assert any(per > 1 and busy < 256 and last == per for per, busy, last in plans)        # trailing threads own nothing
    assert any(per > 1 and busy < 256 and last < per for per, busy, last in plans)         # ... and the last busy one stops short of `per`
    assert any(per > 1 and busy == 256 for per, busy, last in plans)
    assert {(h, w) for _, h, w in L.JPEG_STREAM_CALLS} == set(L.JPEG_SCAN_SHAPES)


def test_jpeg_layout_equals_the_librarys_workspace_query():
    """dts_jpeg_workspace_bytes is host arithmetic: the library loads and answers without a GPU.  The stage tests read the workspace by the
    restated layout, so a changed layout fails here first."""
    from diffusion_tts_amd import _lib
    lib = _lib.load()
    shapes = L.JPEG_STREAM_CALLS + [(1, 16, 16), (3, 16, 32), (64, 512, 512), (64, 1024, 1024), (65535, 16, 16)]
    for n, h, w in shapes:
        lay = L.jpeg_layout(n, h, w)
        assert L.jpeg_shape_ok(n, h, w) and lib.dts_jpeg_workspace_bytes(n, h, w) == lay.bytes, (n, h, w)
        assert lay.coef == 0 and lay.coef < lay.bitoff < lay.totals < lay.bitbuf < lay.bytes
        assert all(v % 256 == 0 for v in lay[1:])
        assert lay.bitoff >= n * lay.nb * 128 and lay.totals - lay.bitoff >= n * lay.nb * 4 and lay.bitbuf - lay.totals >= n * 4
        assert lay.bytes - lay.bitbuf >= n * lay.nb * L.JPEG_BLOCK_BUF_BYTES
    assert L.JPEG_BLOCK_MAX_BITS <= 8 * L.JPEG_BLOCK_BUF_BYTES
    for n, h, w in [(0, 16, 16), (65536, 16, 16), (1, 8, 16), (1, 24, 16), (1, 16, 16400), (2797, 512, 512)]:
        assert not L.jpeg_shape_ok(n, h, w) and lib.dts_jpeg_workspace_bytes(n, h, w) == 0, (n, h, w)
