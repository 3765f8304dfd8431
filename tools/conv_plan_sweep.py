#!/usr/bin/env python3
"""The fixed sweep of dts_conv2d calls behind tests/golden/conv_plan_parent.json.gz (JSON, gzipped: a third of a megabyte of digits otherwise), and its recorder (no GPU).

    python tools/conv_plan_sweep.py --count
    DTS_CONV_DRY=1 python tools/conv_plan_sweep.py --record LIB | gzip -n -9 > tests/golden/conv_plan_parent.json.gz

LIB is a libdts_hip.so of the commit BEFORE the launch plan existed, built with a throw-away patch under which, with DTS_CONV_DRY set,
every launch site (conv kernel, reduce kernel) appends one line -- template arguments, grid, block, LDS bytes, splits, ks_per_split,
whether the kernel gets the statistics pointer, stats_in_reduce, stats_written, epi_rows -- to a buffer that `dts_dry_take()` returns, and
returns before the launch.  The recorder stores, per row, the three queries' answers, dts_conv2d's return code and those lines rewritten
as dts_conv_plan_info's fields.  tests/test_conv_plan.py holds the current library to the file, field for field.

Row: [args, knobs, env, queries, rc, index into "plans" or -1, reduce]; args in ARGS order (pointers as 0 / 1 = absent / present, `ws_mib` =
workspace MiB or -1 for none), knobs a dict of _lib.KNOBS names, env = 1: the row runs with DTS_F32_TILE192=0 (read once per process: its own
process); "plans": the distinct plans in PLAN order; reduce: 0 = no reduce launch, else 2 * SPLITS + with_stats."""
import argparse
import ctypes as C
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, ROOT)

ARGS = ('c1', 'c2', 'n', 'hin', 'win', 'cout', 'ksize', 'up', 'dtype', 'residual', 'gn_coef', 'stats_out', 'out_split2', 'ws_mib', 'skip_c', 'skip_up',
        'skip_ptrs', 'acc_scale')
PLAN = ('kernel', 'tile', 'waves', 'stages', 'pf', 'gn', 'sk', 'dbg', 'splits', 'ks_per_split', 'n_ct', 'n_pt', 'nblk', 'threads', 'lds_bytes',
        'stats_in_kernel', 'stats_in_reduce', 'stats_written', 'epi_rows')
F32, BF16, F16, X3 = 0, 1, 2, 3
MODE = {'f32': F32, 'bf16': BF16, 'f16': F16, 'f16x3': X3}
WS = 96               # MiB


def row(dtype, n, h, w, c1, cout, k=3, c2=0, up=0, res=0, gn=0, stats=0, split2=0, ws=WS, skip=None, acc=0.0, knobs=None, env=0):
    """channel counts as the Python surface sees them: the split-precision launch reads ONE 16-bit source of 2 * (c1 + c2) channels"""
    if dtype == X3:
        c1, c2 = 2 * (c1 + c2), 0
    sc, su, sp = (2 * skip[0], int(skip[1]), int(skip[2]) if len(skip) > 2 else 1) if skip else (0, 0, 0)
    return [[c1, c2, n, h, w, cout, k, int(up), dtype, int(res), int(gn), int(stats), int(split2), ws, sc, su, sp, acc], dict(knobs or {}), env]


def sweep():
    import conv_reference as R
    rows = []
    # every dts_conv2d case of the GPU table in each of its modes with its knobs (what ops.conv2d passes: statistics only for whole strips)
    for c in R.CASES.values():
        if c.form.startswith('in3') or c.form.startswith('out3'):
            continue
        ho, wo = R.out_hw(c)
        for m in c.modes:
            rows.append(row(MODE[m], c.n, c.h, c.w, c.c1, c.cout, c.k, c.c2, c.up, 'r' in c.ep, c.gn, c.stats and (ho * wo) % 64 == 0 and not c.split2,
                            c.split2, WS, c.skip[:2] if c.skip else None, knobs=dict(c.knobs)))
    # the networks' layers: ADM-64 levels (plain, concat input, fused upsample), classifier / VAE widths, DDPM++ 32x32
    shapes = []
    for hw, ch in ((64, 192), (32, 384), (16, 576), (8, 768)):
        shapes += [(hw, ch, 0, ch, 0), (hw, ch, ch, ch, 0), (hw // 2, ch, 0, ch, 1)]
    shapes += [(32, 128, 0, 128, 0), (16, 256, 0, 256, 0), (8, 512, 0, 512, 0), (32, 256, 0, 256, 0), (32, 256, 256, 256, 0)]
    mixes = ((0, 0, WS), (1, 1, WS), (0, 1, -1), (1, 0, 1))          # residual, statistics, workspace: 96 MiB / none / too small for 2 slabs
    for hw, c1, c2, cout, up in shapes:
        for n in (1, 8, 16, 64):
            for k in (3, 1):
                for dt in (F32, BF16, F16, X3):
                    # (all four mixes under the 3x3; F16 differs from BF16 in the element type alone, and a 1x1 never leaves the implicit GEMM)
                    for res, st, ws in (mixes if k == 3 and dt != F16 else (mixes[1], mixes[3] if k == 1 else mixes[2])):
                        rows.append(row(dt, n, hw, hw, c1, cout, k, c2, up, res=res, stats=st, ws=ws))
                rows.append(row(X3, n, hw, hw, c1, cout, k, c2, up, split2=1))
    # ping-pong grids of exactly 63 .. 257 blocks (16x16 images: one 256-pixel tile each; one cout tile), with and without a skip to fold
    for n in (63, 64, 65, 128, 129, 191, 192, 256, 257):
        for cout in (192, 128):
            for dt in (BF16, F16, X3):
                rows.append(row(dt, n, 16, 16, 384, cout, stats=1))
                rows.append(row(dt, n, 16, 16, 384, cout, stats=1, knobs={'conv_variant': 1}))
            rows.append(row(X3, n, 16, 16, 384, cout, skip=(192, 0)))
            rows.append(row(X3, n, 32, 32, 192, cout, skip=(192, 1)))
    # each knob alone
    knobs = [('conv_variant', v) for v in (0, 1, 11, 91)] + [('conv_splits', v) for v in (1, 2, 3, 8, 9)] + [('conv_stages', v) for v in (2, 3, 4)]
    knobs += [('conv_waves', v) for v in (4, 8)] + [('conv_tile', v) for v in (64, 128, 192, 256)] + [('conv_half_round', v) for v in (0, 1)]
    knobs += [('conv_epi32', v) for v in (0, 1, 2)] + [('conv_skip_fold', 0)]
    sub = [(64, 192, 192, 192, 0), (32, 384, 0, 384, 0), (8, 768, 0, 768, 0), (32, 256, 0, 256, 0), (16, 128, 0, 128, 1)]
    for name, v in knobs:
        for hw, c1, c2, cout, up in sub:
            for n in (8, 64):
                for dt in (F32, BF16, F16, X3) if n == 8 else (BF16, X3):
                    rows.append(row(dt, n, hw, hw, c1, cout, 3, c2, up, stats=1, knobs={name: v}))
                    if name in ('conv_splits', 'conv_tile', 'conv_waves', 'conv_stages') and n == 8 and dt != F16:
                        rows.append(row(dt, n, hw, hw, c1, cout, 1, c2, up, res=1, knobs={name: v}))
        if name in ('conv_skip_fold', 'conv_splits', 'conv_variant'):
            for n in (8, 64):
                rows.append(row(X3, n, 32, 32, 384, 384, skip=(768, 0), knobs={name: v}))
    rows.append(row(BF16, 64, 32, 32, 384, 384, gn=1, knobs={'conv_variant': 0}))
    rows.append(row(BF16, 64, 32, 32, 384, 384, gn=1, knobs={'conv_tile': 128}))
    # DTS_F32_TILE192=0
    for cout in (192, 384, 576, 128):
        for n in (1, 64):
            rows.append(row(F32, n, 16, 16, 192, cout, env=1))
            rows.append(row(F32, n, 16, 16, 192, cout, k=1, knobs={'conv_tile': 192}, env=1))
    # fused GroupNorm / folded skip: admitted and refused
    for dt in (BF16, F16, X3, F32):
        for n, hw, ch in ((64, 32, 384), (2, 16, 192), (8, 64, 192), (64, 8, 768), (64, 16, 256)):
            rows.append(row(dt, n, hw, hw, ch, ch, gn=1))
            rows.append(row(dt, n, hw, hw, ch, ch, gn=1, res=1, knobs={'conv_variant': 1}))
            rows.append(row(dt, n, hw, hw, ch, ch, skip=(ch, 0)))
            rows.append(row(dt, n, hw, hw, ch, ch, skip=(ch, 0), res=1))
    rows.append(row(X3, 64, 32, 32, 384, 384, skip=(768, 0, 0)))          # skip_c without the pointers
    rows.append(row(X3, 64, 33, 33, 384, 384, skip=(768, 1)))
    rows.append(row(X3, 64, 32, 32, 384, 384, skip=(48, 0)))
    # invalid arguments
    bad = [dict(k=2), dict(n=0), dict(n=-1), dict(h=0), dict(w=-3), dict(cout=0), dict(cout=-192), dict(cout=100), dict(cout=32), dict(c1=0), dict(c1=48),
           dict(c1=96), dict(c2=16), dict(n=1 << 20, h=64, w=64), dict(n=1 << 18, h=32, w=32, up=1), dict(c1=40000), dict(c1=1 << 20), dict(h=40000, w=1, n=1),
           dict(split2=1), dict(split2=1, stats=1), dict(acc=0.5), dict(acc=1.0), dict(k=0), dict(dtype=7)]
    for b in bad:
        for dt in (F32, BF16, X3):
            for kn in ({}, {'conv_variant': 1}) if set(b) & {'n', 'h', 'w', 'cout', 'c1'} else ({},):
                kw = dict(n=4, h=16, w=16, c1=192, cout=192, knobs=kn)
                kw.update(b)
                rows.append(row(kw.pop('dtype', dt), kw.pop('n'), kw.pop('h'), kw.pop('w'), kw.pop('c1'), kw.pop('cout'), **kw))
                rows.append(row(dt, 4, 16, 16, 192, 192, gn=1, **{k_: v for k_, v in b.items() if k_ in ('k', 'c2', 'split2', 'acc')}, knobs=kn))
    seen, out = set(), []
    for r in rows:
        key = json.dumps(r, sort_keys=True)
        if key not in seen:
            seen.add(key)
            out.append(r)
    return out


def conv_args(L, a):
    """a _lib.ConvArgs of a row's args (any non-null pointer will do: the host never dereferences one)"""
    d = dict(zip(ARGS, a))
    ca, ptr = L.ConvArgs(), 0x1000
    for f in ('c1', 'c2', 'n', 'hin', 'win', 'cout', 'ksize', 'up', 'dtype', 'out_split2', 'skip_c', 'skip_up'):
        setattr(ca, f, d[f])
    ca.x1 = ca.w = ca.out = ptr
    ca.x2 = ptr if d['c2'] else None
    for f in ('residual', 'gn_coef', 'stats_out'):
        setattr(ca, f, ptr if d[f] else None)
    ca.skip_x = ca.skip_w = ptr if d['skip_ptrs'] else None
    ca.workspace, ca.workspace_bytes = (None, 0) if d['ws_mib'] < 0 else (ptr, d['ws_mib'] << 20)
    ca.out_scale, ca.acc_scale = 1.0, d['acc_scale']
    return ca


CONV_KNOBS = ('conv_tile', 'conv_splits', 'conv_variant', 'conv_stages', 'conv_waves', 'conv_half_round', 'conv_epi32', 'conv_skip_fold')


def set_knobs(L, lib, knobs):
    for k in CONV_KNOBS:
        lib.dts_set_tuning(L.KNOBS[k], int(knobs.get(k, -1)))


def parse(lines, dtype):
    """the dry-run lines of one dts_conv2d call -> (plan fields in PLAN order, [SPLITS, with_stats] of the reduce launch or None)"""
    f = lambda ln: {k: v for k, v in re.findall(r'(\w+)=(-?[\d,]+)', ln)}
    meta = conv = red = None
    for ln in lines:
        kind, d = ln.split()[0], f(ln)
        if kind == 'meta':
            meta = d
        elif kind == 'reduce':
            red = d
        else:
            conv = (kind, d)
    kind, d = conv
    gx, gy = (int(v) for v in d['grid'].split(','))
    i = lambda k: int(d[k])
    code = {F32: (0, 0), BF16: (1, 1), F16: (2, 2), X3: (2, 0)}[dtype]
    assert (i('T'), i('OT')) == code and gy == i('splits') and gx == i('n_ct') * i('n_pt'), (lines, dtype)
    if kind == 'igemm':
        assert i('NT') == 4
        head = [0, 16 * i('MT') * i('WM'), i('WM') * i('WN'), i('STAGES'), i('PF'), 0, 0, 0]
    else:
        assert i('TAPS') == 9
        head = [i('MT'), 0, 0, 0, 0, i('GN'), i('SK'), i('DBG')]
    plan = head + [i('splits'), i('ks'), i('n_ct'), i('n_pt'), gx, i('block'), i('lds'), i('stats'), int(meta['stats_in_reduce']),
                   int(meta['stats_written']), i('epi_rows')]
    r = None
    if red is not None:
        r = [int(red['SPLITS']), int(red['with_stats'])]
        assert int(red['OT']) == code[1] and int(red['stats']) == int(red['with_stats'])
    assert (r is not None) == (i('splits') > 1)
    return plan, r


def record(lib_path, env):
    os.environ['DTS_LIB_PATH'] = lib_path
    from diffusion_tts_amd import _lib as L
    lib = C.CDLL(lib_path)
    lib.dts_dry_take.restype = C.c_char_p
    lib.dts_conv_kernel.restype = lib.dts_conv_fuses_gn.restype = lib.dts_conv_folds_skip.restype = lib.dts_conv2d.restype = C.c_int
    out = []
    for a, knobs, e in sweep():
        if e != env:
            continue
        set_knobs(L, lib, knobs)
        ca = conv_args(L, a)
        q = [lib.dts_conv_kernel(C.byref(ca)), lib.dts_conv_fuses_gn(C.byref(ca)), lib.dts_conv_folds_skip(C.byref(ca))]
        lib.dts_dry_take()
        rc = lib.dts_conv2d(C.byref(ca), None)
        lines = lib.dts_dry_take().decode().splitlines()
        plan, red = parse(lines, a[ARGS.index('dtype')]) if rc == 0 else (None, None)
        assert rc != 0 or (plan[PLAN.index('stats_written')] == ca.stats_written and plan[0] == q[0]), (a, knobs, lines)
        out.append([a, knobs, e, q, rc, plan, red])
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--count', action='store_true')
    ap.add_argument('--record', metavar='LIB')
    ap.add_argument('--env', type=int, default=-1, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.count:
        print(len(sweep()))
        return
    assert os.environ.get('DTS_CONV_DRY'), 'set DTS_CONV_DRY=1: without it the patched library launches'
    if a.env >= 0:
        print(json.dumps(record(a.record, a.env)))
        return
    rows = []
    for e in (0, 1):
        env = dict(os.environ, **({'DTS_F32_TILE192': '0'} if e else {}))
        rows += json.loads(subprocess.run([sys.executable, __file__, '--record', a.record, '--env', str(e)], env=env, check=True,
                                          capture_output=True, text=True).stdout)
    plans = sorted({tuple(r[5]) for r in rows if r[5] is not None})
    index = {p: i for i, p in enumerate(plans)}
    rows = [[[int(v) if v == int(v) else v for v in a], k, e, q, rc, -1 if p is None else index[tuple(p)], 0 if red is None else 2 * red[0] + red[1]]
            for a, k, e, q, rc, p, red in rows]
    dump = lambda items, per: ',\n'.join(','.join(json.dumps(x, separators=(',', ':')) for x in items[i:i + per]) for i in range(0, len(items), per))
    print('{"args": %s,\n "plan": %s,\n "plans": [\n%s],\n "rows": [\n%s]}' % (json.dumps(ARGS), json.dumps(PLAN), dump(plans, 4), dump(rows, 3)))


if __name__ == '__main__':
    main()
