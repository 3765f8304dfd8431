"""GPU: ops.group_rows (dts_group_rows) -- the groups of bitwise-identical rows of a device matrix, numbered in order of first occurrence --
against a numpy reference over the bytes of every row (`tobytes()`, a dictionary of first occurrences).  The comparison is exact: the kernel
is integer-only and confirms every fingerprint match byte for byte, so slot, reps and count have one right answer.

Cases: one row; the search loop's pattern [a,a,b,a,a,b]; 64 rows all distinct / all equal; 33 rows (not a multiple of the wave) whose
differences from row 0 sit in the last two or in the first two bytes only (the ends of the first and the last 16-byte vector of a lane's walk);
+0.0 against -0.0 (equal as numbers, different bytes); rows of 16 bytes (one vector), 16*37 (fewer vectors than one wave pass), 77*768*2 (SD-1.5's
text context: 29 passes of the 256-thread fingerprint block, 116 of the comparing wave); and the maximum of 1024 rows, where every wave of
the grouping block walks 64 rows and a candidate search spans 16 ballots."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = 'cuda'


def reference(rows_u8):
    """first-occurrence grouping over the bytes of each row: (slot [n], reps [n] padded with -1, count)"""
    seen, slot, reps = {}, [], []
    for i, r in enumerate(rows_u8):
        key = r.tobytes()
        if key not in seen:
            seen[key] = len(reps)
            reps.append(i)
        slot.append(seen[key])
    n = len(rows_u8)
    return np.array(slot, dtype=np.int32), np.array(reps + [-1] * (n - len(reps)), dtype=np.int32), len(reps)


def random_rows(n, row_bytes, seed):
    return np.random.default_rng(seed).integers(0, 256, size=(n, row_bytes), dtype=np.uint8)


def case_rows(name):
    if name == 'one_row':
        return random_rows(1, 16 * 37, 1)
    if name == 'aabaab':
        a, b = random_rows(2, 16 * 37, 2)
        return np.stack([a, a, b, a, a, b])
    if name == 'distinct64':
        return random_rows(64, 16 * 37, 3)
    if name == 'equal64':
        return np.repeat(random_rows(1, 16 * 37, 4), 64, axis=0)
    if name == 'ends33':
        # row 0 and copies of it; copies changed in the last two bytes only (two variants); copies changed in the first two bytes only
        rows = np.repeat(random_rows(1, 16 * 37, 5), 33, axis=0)
        for i in range(1, 33):
            kind = i % 4
            if kind == 1:
                rows[i, -2:] ^= np.array([0x01, 0x80], dtype=np.uint8)
            elif kind == 2:
                rows[i, -2:] ^= np.array([0x00, 0x01], dtype=np.uint8)
            elif kind == 3:
                rows[i, :2] ^= np.array([0x40, 0x00], dtype=np.uint8)
        return rows
    if name == 'signed_zero':
        z = np.zeros((6, 8), dtype=np.float16)            # 16 bytes per row
        z[1, 3] = -0.0
        z[3, 3] = -0.0
        z[4, 7] = -0.0
        return z.view(np.uint8).reshape(6, 16)
    if name == 'bytes16':
        rows = random_rows(9, 16, 6)
        rows[5], rows[8] = rows[2], rows[0]
        return rows
    if name == 'sd15_context':
        rows = random_rows(3, 77 * 768 * 2, 7)
        rows = rows[[0, 1, 0, 2, 1, 0, 0]].copy()
        rows[5, -1] ^= 1                                   # one bit in the last byte of 118 272: a group of its own
        return rows
    if name == 'max1024':
        base = random_rows(300, 16, 8)
        idx = np.random.default_rng(9).integers(0, 300, size=1024)
        return base[idx].copy()
    raise KeyError(name)


CASES = ['one_row', 'aabaab', 'distinct64', 'equal64', 'ends33', 'signed_zero', 'bytes16', 'sd15_context', 'max1024']


@pytest.mark.parametrize('name', CASES)
def test_group_rows_matches_first_occurrence_reference(name):
    from diffusion_tts_amd import ops
    rows = case_rows(name)
    n = rows.shape[0]
    want_slot, want_reps, want_count = reference(rows)
    if name == 'signed_zero':
        assert want_count == 3 and list(want_slot) == [0, 1, 0, 1, 2, 0]      # -0.0 is not +0.0 here
    if name == 'ends33':
        assert want_count == 4
    x = torch.from_numpy(rows).to(DEV)
    runs = []
    for _ in range(2):
        slot, reps, count = ops.group_rows(x)
        assert slot.dtype == reps.dtype == count.dtype == torch.int32
        assert tuple(slot.shape) == (n,) and tuple(reps.shape) == (n,) and tuple(count.shape) == (1,)
        runs.append((slot.cpu().numpy().copy(), reps.cpu().numpy().copy(), int(count.cpu()[0])))
    slot, reps, count = runs[0]
    print(f'group_rows {name}: {n} rows of {rows.shape[1]} bytes, {count} groups (reference {want_count})')
    assert count == want_count
    assert np.array_equal(slot, want_slot)
    assert np.array_equal(reps[:count], want_reps[:want_count]) and (reps[count:] == -1).all()
    assert runs[1][2] == count and np.array_equal(runs[1][0], slot) and np.array_equal(runs[1][1], reps)


def test_group_rows_takes_the_model_dtypes_and_trailing_dimensions():
    """the U-Net's use: a [n, L, cd] float16 / bfloat16 tensor, grouped over the bytes of [L, cd]"""
    from diffusion_tts_amd import ops
    g = torch.Generator().manual_seed(3)
    c = torch.randn(2, 11, 64, generator=g)
    for dt in (torch.float16, torch.bfloat16):
        x = torch.cat([c[:1].expand(3, -1, -1), c[1:].expand(3, -1, -1)]).to(DEV, dt).contiguous()
        slot, reps, count = ops.group_rows(x)
        assert slot.tolist() == [0, 0, 0, 1, 1, 1] and reps.tolist() == [0, 3, -1, -1, -1, -1] and count.tolist() == [2]


def test_group_rows_refusals():
    from diffusion_tts_amd import ops
    with pytest.raises(ValueError):
        ops.group_rows(torch.zeros(4, 16, dtype=torch.uint8))                      # a CPU tensor
    with pytest.raises(ValueError):
        ops.group_rows(torch.zeros(4, 24, dtype=torch.uint8, device=DEV))          # 24 bytes per row
    with pytest.raises(ValueError):
        ops.group_rows(torch.zeros(1025, 16, dtype=torch.uint8, device=DEV))       # more rows than the grouping block has threads
