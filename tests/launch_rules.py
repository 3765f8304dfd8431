"""Host launch rules restated in Python, and the cases that take the SECOND trip of the loops those rules size.

Several kernels contain a loop whose trip count the host launcher derives from the problem size; at the small shapes the references
like, every such loop runs once.  Nothing reports which form ran, so each rule is written out here a second time, from the launcher's
text, and the tables below say what each case must reach.  tests/test_launch_rules.py asserts the tables against the rules on the CPU (a
changed cap or heuristic in the library has to be restated here, and then fails there unless the shapes still pass it); the GPU files
assert the same per case and run the kernels.  (The convolutions' rules live with their cases in tests/conv_reference.py.)  Plain Python:
no torch, nothing of diffusion_tts_amd."""
import collections


def ceil_div(a, b):
    return -(-a // b)


# ---- dts_cross_attention (csrc/transformer.hip) -----------------------------------------------------------------------------------------
def xattn_plan(n, heads, tq):
    """(chunks of 64 queries, qchunks = chunks a block walks, qblocks = blocks per (sample, head)): qchunks doubles, up to 8, while
    n * heads * ceil(chunks / (2 * qchunks)) >= 1024 -- the staging of K / V is shared as widely as still leaves ~4 blocks per CU"""
    nh, chunks, qchunks = n * heads, ceil_div(tq, 64), 1
    while qchunks < 8 and nh * ceil_div(chunks, 2 * qchunks) >= 1024:
        qchunks *= 2
    return chunks, qchunks, ceil_div(chunks, qchunks)


XAttn = collections.namedtuple('XAttn', 'n heads d tq tk contexts chunks qchunks qblocks')
# every tq leaves a ragged last chunk (tq % 64 != 0) and a last block with chunks past the end (the wave-uniform `break`)
XATTN_CHUNK_LOOP = [
    XAttn(8, 16, 64, 1030, 77, None, 17, 2, 9),         # the last block holds chunk 16 alone: 6 queries, waves 1..3 break at once
    XAttn(8, 16, 64, 1800, 77, None, 29, 4, 8),         # the last block holds chunk 28 (8 queries) and three chunks past the end
    XAttn(64, 16, 64, 513, 128, None, 9, 8, 2),         # the second block holds chunk 8 (1 query) and seven chunks past the end
    XAttn(64, 16, 64, 581, 77, 2, 10, 8, 2),            # kv_rows over 2 contexts; chunks 8 and 9 (5 queries) in the second block
    XAttn(64, 2, 256, 1030, 77, None, 17, 2, 9),        # d = 256: 16 output tiles per chunk, 102 KiB of LDS at 77 (96 staged) keys
]


# ---- gn_apply_impl (csrc/groupnorm.hip) ----------------------------------------------------------------------------------------------------
GnApply = collections.namedtuple('GnApply', 'kernel k ppb blocks trips last_block_pixels threads w16')
GN_GRID_CAP = 4096          # blocks of 256 threads: grid_for()


def gn_apply_plan(n, c1, c2, h, w, f32, pool=False, split=False, gn_fuse=-1):
    """Which apply kernel serves a shape and how many trips its loop makes.
    rows (gn_apply_rows_kernel): unpooled, at most 256 16-byte chunks per pixel.  k = 256 // chunks pixels per block pass; a block owns ppb =
    ceil(n * hw / 4096) pixels of one sample, rounded up to a multiple of 2k; a thread walks its pixels two per trip (p and p + k, then
    p += 2k) and a single one at the end of a ragged last block.  trips = ppb / 2k, the pair trips of a thread in a whole block.  w16 (split
    image only): the 16-byte lane-pair store form, taken iff c1 % 8 == 0 and gn_fuse != 2.
    grid (gn_apply_kernel): every pooled apply and every wider row; one thread per chunk of an OUTPUT pixel, grid-stride over at most 4096
    blocks of 256.  trips = the most a thread makes."""
    c = c1 + c2
    chunks = c // (4 if f32 else 8)
    if pool or chunks > 256 or n > 65535:
        ho, wo = (h // 2, w // 2) if pool else (h, w)
        threads = n * ho * wo * chunks
        blocks = max(1, min(ceil_div(threads, 256), GN_GRID_CAP))
        return GnApply('grid', None, None, blocks, ceil_div(threads, 256 * blocks), None, threads, None)
    k, hw = 256 // chunks, h * w
    ppb = ceil_div(ceil_div(n * hw, 4096), 2 * k) * 2 * k
    bx = ceil_div(hw, ppb)
    return GnApply('rows', k, ppb, (bx, n), ppb // (2 * k), hw - (bx - 1) * ppb, None, bool(split and c1 % 8 == 0 and gn_fuse != 2))


GnCase = collections.namedtuple('GnCase', 'n c1 c2 h w dtypes pool expect')
# expect: the fields of GnApply the case must reach (the others are not pinned)
GN_ROWS_TWO_TRIPS = {
    # k = 1: 1024 blocks of 4 pixels per sample; the last has 3: one pair and the single-pixel tail
    'c1024': GnCase(3, 1024, 0, 65, 63, ('f32',), False, dict(kernel='rows', k=1, ppb=4, trips=2, last_block_pixels=3)),
    # k = 3: 1036 whole blocks of 12 pixels
    'c576': GnCase(2, 576, 0, 112, 111, ('bf16', 'f16'), False, dict(kernel='rows', k=3, ppb=12, trips=2, last_block_pixels=12)),
    # k = 5: 418 blocks of 20 pixels and one of 12: a pair for every pixel row, then the tail for rows 0 and 1
    'c192': GnCase(5, 192, 0, 92, 91, ('f32',), False, dict(kernel='rows', k=5, ppb=20, trips=2, last_block_pixels=12)),
    # the same tensor as a concat whose first half is no multiple of 8 channels: the split image's 8-byte store form whatever the knob says
    'c100+92': GnCase(5, 100, 92, 92, 91, ('f32',), False, dict(kernel='rows', k=5, ppb=20, trips=2, last_block_pixels=12)),
}
GN_GRID_TWO_TRIPS = {
    # 4096 * 256 = 1,048,576 threads per trip
    'pool_f32': GnCase(2, 192, 0, 50, 874, ('f32',), True, dict(kernel='grid', blocks=4096, trips=2, threads=1048800)),         # + 224
    'pool_16bit': GnCase(4, 192, 0, 50, 874, ('bf16', 'f16'), True, dict(kernel='grid', blocks=4096, trips=2, threads=1048800)),   # + 224
    'wide_f32': GnCase(1, 1536, 0, 1, 2731, ('f32',), False, dict(kernel='grid', blocks=4096, trips=2, threads=1048704)),       # + 128
}


# ---- dts_layer_norm / dts_vit_head (csrc/transformer.hip, csrc/vit.hip) ---------------------------------------------------------------------
def layer_norm_vectors(c):
    """register vectors (8 channels per lane, 64 lanes) of a row: which of the four `i` iterations of the 16-bit kernels hold data, and how
    many lanes of the last one"""
    nvec = c // 8
    return ceil_div(nvec, 64), nvec - 64 * (ceil_div(nvec, 64) - 1)


# c -> (register vectors in use, lanes of the last one): 8 is the single-lane row, 1544 the fourth vector on ONE lane, 2048 all four whole
LAYER_NORM_WIDTHS = {8: (1, 1), 1544: (4, 1), 2048: (4, 64)}


# ---- dts_jpeg_size (csrc/jpeg.hip) ------------------------------------------------------------------------------------------------------------
JPEG_BLOCK_BUF_BYTES = 256          # bit-buffer bytes per 8x8 block (kBlockBufBytes)
JPEG_BLOCK_MAX_BITS = 64 * (16 + 11)     # the most a block costs: 64 coefficients of a 16-bit code and 11 value bits (kBlockMaxBits)
JpegLayout = collections.namedtuple('JpegLayout', 'nb coef bitoff totals bitbuf bytes')


def align256(x):
    return (x + 255) & ~255


def jpeg_layout(n, h, w):
    """byte offsets of the workspace's four arrays (layout() of the host part): int16 coefficients [n][nb][64], int bit counts / offsets
    [n][nb], int totals [n], the bit buffer of 256 bytes per block; every array starts on a multiple of 256 bytes"""
    nb = (h // 16) * (w // 16) * 6
    blocks = n * nb
    coef = 0
    bitoff = coef + align256(blocks * 128)
    totals = bitoff + align256(blocks * 4)
    bitbuf = totals + align256(n * 4)
    return JpegLayout(nb, coef, bitoff, totals, bitbuf, bitbuf + align256(blocks * JPEG_BLOCK_BUF_BYTES))


def jpeg_shape_ok(n, h, w):
    """shape_ok() of the host part: whole MCUs, the caps on n, h, w and on all blocks of a call, and the bits of one image's scan -- at the
    most a block can cost -- below 2^31, because bit counts, offsets and positions are int"""
    mcus = (h // 16) * (w // 16)
    return (1 <= n <= 65535 and h >= 16 and w >= 16 and h % 16 == 0 and w % 16 == 0 and h <= 16384 and w <= 16384
            and n * mcus * 6 <= 1 << 24 and mcus * 6 * JPEG_BLOCK_MAX_BITS < 1 << 31)


def jpeg_scan_plan(nb):
    """jpeg_scan_kernel, one workgroup of 256 threads per image: (per = blocks a thread sums and rewrites, busy = threads that own at least
    one block, last = blocks of the last busy thread); thread t owns [min(t * per, nb), min(t * per + per, nb))"""
    per = ceil_div(nb, 256)
    busy = ceil_div(nb, per)
    return per, busy, nb - (busy - 1) * per


# (h, w) -> (nb, per, busy, last) of every shape the stream tests run: one block per thread with idle threads (nb <= 256), 2 and 3 per
# thread with the upper threads clamped to nothing, 4 per thread with a last busy thread that owns 2 (the only clamp of `hi`: nb is a
# multiple of 6, so per = 2 and 3 divide it), and 24 per thread with every thread busy
JPEG_SCAN_SHAPES = {
    (16, 16): (6, 1, 6, 1),
    (32, 32): (24, 1, 24, 1),
    (64, 64): (96, 1, 96, 1),
    (48, 80): (90, 1, 90, 1),
    (80, 48): (90, 1, 90, 1),
    (112, 112): (294, 2, 147, 2),
    (176, 160): (660, 3, 220, 3),
    (48, 688): (774, 4, 194, 2),
    (512, 512): (6144, 24, 256, 24),
}
# (n, h, w) of every call of the stream tests
JPEG_STREAM_CALLS = [(9, 16, 16), (9, 48, 80), (9, 80, 48), (9, 112, 112), (9, 176, 160), (9, 48, 688), (1, 512, 512), (9, 32, 32),
                     (1, 64, 64), (5, 64, 64), (64, 64, 64)]
