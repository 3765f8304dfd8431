"""A batch past 2^31 and 2^32 bytes made of K = 7 distinct samples: the map, the tiling, the class-wise bit comparison and the byte
bookkeeping (tests/test_gpu_large_rows.py runs the kernels; tests/test_large_rows_cpu.py holds this file and the case table
launch_rules.LARGE_CASES to account on the CPU).

Every kernel here is independent per sample, so a batch of n rows needs no reference of n rows.  Row i of the input is base sample
idx[i], idx a SEEDED RANDOM map [n] -> {0..6} (row_map: torch.Generator; never i % 7, so that a result that lands a fixed number of
samples away from where it belongs -- an index that wrapped at 2^32 bytes or 2^31 elements -- lands on another base).  After ONE launch
    - every row with idx == k must be BIT-equal to the first such row (class_mismatches: an integer view, in chunks, no second copy of the
      tensor): identical rows at different batch positions give identical bits, at every position up to the end;
    - the first row of each class is held to the kernel's own reference by the caller (7 rows);
    - the output is the middle of a NaN-filled buffer (guarded) whose bands must still be NaN (bands_intact), and no first row may hold a
      NaN the reference does not: with the bit equality every element of every row was then written.
The byte bookkeeping (crossings, sample_at_byte, samples_beyond, wrap_distances) is plain Python: no torch until a function is called."""
K = 7
SEED = 65
GUARD = 4096
B31, B32 = 1 << 31, 1 << 32
BOUNDARIES = ('byte31', 'byte32', 'elem31')


# ---- byte bookkeeping (plain Python) ------------------------------------------------------------------------------------------------------
def numel(shape):
    m = 1
    for s in shape:
        m *= s
    return m


def boundary_byte(which, itemsize):
    """the byte offset at which a tensor of `itemsize`-byte elements reaches the boundary: byte 2^31, byte 2^32, element 2^31"""
    return {'byte31': B31, 'byte32': B32, 'elem31': B31 * itemsize}[which]


def crossings(nbytes, itemsize):
    """which of the three boundaries lie strictly inside a tensor of nbytes (an offset AT the boundary is addressed)"""
    return tuple(b for b in BOUNDARIES if nbytes > boundary_byte(b, itemsize))


def sample_at_byte(byte, sample_bytes):
    return byte // sample_bytes


def samples_beyond(n, sample_bytes, byte):
    """whole samples that lie entirely at or beyond `byte`"""
    return n - -(-byte // sample_bytes)


def wrap_distances(sample_bytes, itemsize):
    """the whole numbers of samples by which an index that lost its bit 32 (bytes) or bit 31 / 32 (elements) is displaced"""
    out = []
    for span in (B32, B31 * itemsize, B32 * itemsize, B31):
        if span % sample_bytes == 0 and span // sample_bytes not in out:
            out.append(span // sample_bytes)
    return out


# ---- the map ----------------------------------------------------------------------------------------------------------------------------------
def row_map(n, seed=SEED):
    """idx [n] int64 in {0..6}: seeded, random, every class present"""
    import torch
    idx = torch.randint(0, K, (n,), generator=torch.Generator().manual_seed(seed))
    assert n < K or len(torch.unique(idx)) == K
    return idx


def first_rows(idx):
    """[K]: the first row of each class"""
    import torch
    return torch.stack([(idx == k).nonzero()[0, 0] for k in range(K)])


def map_separates(idx, n, sample_bytes, itemsize):
    """The property that keeps a systematic shift from passing by coincidence, per boundary the tensor crosses: the sample s that holds the
    boundary byte has another base than sample 0, and another base than the samples s - d and s + d for every wrap distance d.  Returns
    the list of violations (empty = separated)."""
    bad = []
    for b in crossings(n * sample_bytes, itemsize):
        s = sample_at_byte(boundary_byte(b, itemsize), sample_bytes)
        if int(idx[s]) == int(idx[0]):
            bad.append((b, s, 0))
        for d in wrap_distances(sample_bytes, itemsize):
            for t in (s - d, s + d):
                if 0 <= t < n and int(idx[t]) == int(idx[s]):
                    bad.append((b, s, t))
    return bad


# ---- tiling -------------------------------------------------------------------------------------------------------------------------------------
def tile(base, idx, out=None):
    """x = base[idx]: base [K, ...] -> [n, ...] on base's device (one gather, no intermediate; into `out` where given)"""
    import torch
    assert base.shape[0] == K
    return torch.index_select(base, 0, idx.to(base.device), out=out)


FILL_U8 = 0xA5


def guarded(shape, dtype, device, guard=GUARD):
    """an output tensor in the middle of a NaN-filled buffer (integer types: filled with 0xA5): (buffer, view)"""
    import torch
    m = numel(shape)
    buf = torch.full((m + 2 * guard,), float('nan') if dtype.is_floating_point else FILL_U8, dtype=dtype, device=device)
    return buf, buf[guard:guard + m].view(shape)


def _is_fill(t):
    import torch
    return torch.isnan(t) if t.dtype.is_floating_point else t == FILL_U8


def bands_intact(buf, guard=GUARD):
    return bool(_is_fill(buf[:guard]).all()) and bool(_is_fill(buf[-guard:]).all())


# ---- the comparison ---------------------------------------------------------------------------------------------------------------------------
_INT = {1: 'int8', 2: 'int16', 4: 'int32', 8: 'int64'}


def int_rows(t):
    """[n, m] integer view of a contiguous [n, ...] tensor: bits, so that NaNs compare equal and -0.0 differs from 0.0"""
    import torch
    assert t.is_contiguous()
    return t.view(t.shape[0], -1).view(getattr(torch, _INT[t.element_size()]))


def class_mismatches(out, idx, chunk_bytes=64 << 20, limit=8):
    """Rows of `out` [n, ...] whose bits differ from the first row of their class: a list of (row, class, first differing element in the
    row), at most `limit`, walking the tensor in chunks of about chunk_bytes.  Empty = every class is bit-identical throughout."""
    import torch
    rows = int_rows(out)
    idx = idx.to(out.device)
    ref = rows[first_rows(idx).to(out.device)]                     # [K, m]
    n, m = rows.shape
    step = max(1, chunk_bytes // max(1, m * out.element_size()))
    bad = []
    for r0 in range(0, n, step):
        ne = rows[r0:r0 + step] != ref[idx[r0:r0 + step]]
        hit = ne.any(1)
        if bool(hit.any()):
            for r in hit.nonzero()[:, 0].tolist():
                bad.append((r0 + r, int(idx[r0 + r]), int(ne[r].nonzero()[0, 0])))
                if len(bad) >= limit:
                    return bad
    return bad


def assert_classes_bit_equal(out, idx, what=''):
    bad = class_mismatches(out, idx)
    assert not bad, f'{what}: rows differ from the first row of their class (row, class, element): {bad}'


def first_of_classes(out, idx):
    """the K rows the reference judges, on the CPU: out[first_rows(idx)]"""
    return out[first_rows(idx).to(out.device)].cpu()
