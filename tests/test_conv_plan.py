"""CPU: the launch plan of dts_conv2d (dts_conv_plan) and the three queries that read it against the decisions of the commit before the
plan existed, recorded as data: tests/golden/conv_plan_parent.json.gz (tools/conv_plan_sweep.py says how it was recorded and defines the
sweep -- every dts_conv2d case of conv_reference.CASES with its knobs, the networks' layers at 1 / 8 / 16 / 64 rows in all four dtypes,
ping-pong grids of 63 .. 257 blocks, each knob alone, invalid arguments).  Host logic only: no GPU, no tolerance, no row left out.
Per row: dts_conv_kernel / dts_conv_fuses_gn / dts_conv_folds_skip equal the recording; where the recorded dts_conv2d returned an error
the plan is refused (and so are the rows that launched the retired variant 91); otherwise every field of the plan equals what the recorded
launch site was given (template arguments, grid, block, LDS bytes, splits, ks_per_split, who writes the statistics, epi_rows) and a reduce launch follows exactly where one was recorded."""
import ctypes as C
import gzip
import json
import os
import subprocess
import sys

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, 'tools'))
import conv_plan_sweep as S  # noqa: E402

GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'conv_plan_parent.json.gz')


def check_rows(env):
    """every row of the recording with this `env` flag against the library; returns how many were compared"""
    from diffusion_tts_amd import _lib as L
    lib = L.load()
    with gzip.open(GOLDEN, 'rt') as f:
        gold = json.load(f)
    assert tuple(gold['args']) == S.ARGS and tuple(gold['plan']) == S.PLAN
    old = {k: int(lib.dts_get_tuning(L.KNOBS[k])) for k in S.CONV_KNOBS}
    count = 0
    try:
        for a, knobs, e, q, rc, plan, red in gold['rows']:
            if e != env:
                continue
            plan = None if plan < 0 else gold['plans'][plan]
            S.set_knobs(L, lib, knobs)
            ca, info, what = S.conv_args(L, a), L.ConvPlanInfo(), (a, knobs)
            got_q = [lib.dts_conv_kernel(C.byref(ca)), lib.dts_conv_fuses_gn(C.byref(ca)), lib.dts_conv_folds_skip(C.byref(ca))]
            assert got_q == q, (what, got_q, q)
            st = lib.dts_conv_plan(C.byref(ca), C.byref(info))
            assert st == (-1 if q[0] < 0 else 0), what
            assert [info.kernel, info.fuses_gn, info.folds_skip] == q, what
            if plan is not None and plan[S.PLAN.index('dbg')] == 9:
                # the one intended difference: DTS_CONV_VARIANT=91 (conv_pp_kernel<.., DBG = 9>, an experiment measured slower) was compiled into
                # the product library when the recording was made; it now exists in -DDTS_DIAG_KERNELS builds only and is refused like 11 .. 81
                assert info.refused == 1 and b'DTS_DIAG_KERNELS' in lib.dts_last_error(), what
                count += 1
                continue
            assert info.refused == (rc != 0), (what, lib.dts_last_error())
            if rc == 0:
                got = [int(getattr(info, f)) for f in S.PLAN]
                assert got == plan, (what, dict(zip(S.PLAN, got)), dict(zip(S.PLAN, plan)))
                assert red == (2 * info.splits + info.stats_in_reduce if info.splits > 1 else 0), what
            count += 1
    finally:
        S.set_knobs(L, lib, {k: v for k, v in old.items() if v != -1})
    return count


def test_plan_and_queries_equal_the_recorded_parent():
    """(the file is a recording: it holds the sweep as it was when it was made, conv_reference.CASES of that day included, and stays as it is)"""
    assert os.path.getsize(GOLDEN) < (1 << 20)
    assert check_rows(0) == 3257


def test_f32_tile192_rows_in_their_own_process():
    """DTS_F32_TILE192 is read once per process: its rows run in a child whose environment sets it (this test is about exactly that)"""
    r = subprocess.run([sys.executable, '-c', 'import test_conv_plan as t; print("rows", t.check_rows(1))'], cwd=os.path.dirname(__file__),
                       env=dict(os.environ, DTS_F32_TILE192='0'), capture_output=True, text=True)
    assert r.returncode == 0 and 'rows 16' in r.stdout, r.stdout + r.stderr
