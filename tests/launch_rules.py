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
